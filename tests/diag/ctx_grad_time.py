"""Diagnostic (by hand, one MI355X): what the prompt-state gradient costs at Stable Diffusion's size (profiles/null_text.md).
    python tests/diag/ctx_grad_time.py [out.md] [--calls N]
SD15_UNET (64 x 64 latent, 77 x 768 states) with seeded weights, bf16x3, k = 1, warm.  pmp_vjp without and with context_grad
interleaved call by call; one inner iteration of null-text inversion (set_context, primal, eps, guided step, loss, cotangent,
Adam); the device-to-device copy rate of the same box.  Every figure is the median of 7 timed calls after 2 untimed ones, by
device events around the call.  `--calls N` instead runs N pmp_vjp(context_grad=True) calls and nothing else: the run to put
under a kernel trace, whose per-dispatch durations give the new kernels' share per level (the grid's x size is the number of
64-token blocks of the level)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd.config import SD15_UNET, synth_params  # noqa: E402
from loco_edit_amd.hip import LocoEngine  # noqa: E402
from loco_edit_amd.null_text import eps_coefficient  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(xs):
    return f"{statistics.median(xs):.3f} | {min(xs):.3f} - {max(xs):.3f}"


def stage_bytes(cfg):
    """Per level: (tokens, channels, stages, bytes the two new kernels must move per stage: q, g_o and the 80 held columns of P
    read once, the token-block partials written and read once)."""
    out, C = [], cfg.ch
    LW, nres = 80, cfg.num_res_blocks
    for lvl, m in enumerate(cfg.ch_mult):
        res, C = cfg.resolution >> lvl, cfg.ch * m
        if res not in cfg.attn_resolutions:
            continue
        T, NH = res * res, cfg.num_heads
        n = nres + (nres + 1)
        out.append((T, C, n, 4 * (2 * C * T + NH * T * LW) + 2 * 4 * (T // 64) * 2 * C * LW))
    T = (cfg.resolution >> (len(cfg.ch_mult) - 1)) ** 2
    out.append((T, C, 1, 4 * (2 * C * T + cfg.num_heads * T * LW) + 2 * 4 * (T // 64) * 2 * C * LW))
    return out


def main():
    argv = sys.argv[1:]
    calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 0
    outp = argv[0] if argv and not argv[0].startswith("--") else None
    cfg = SD15_UNET
    eng = LocoEngine(cfg, max_batch=1, device=DEV)
    eng.load_state_dict(synth_params(cfg, 0))
    eng.set_precision("bf16x3")
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, 4, 64, 64, generator=g).to(DEV)
    null = torch.randn(77, 768, generator=g).to(DEV)
    U = torch.randn(1, cfg.n, generator=g).to(DEV)
    t, at, at_next = 703.0, 0.19, 0.2
    eng.set_context(null)
    eng.pmp_primal(z, t, at, None, use_et=True)
    if calls:
        for _ in range(calls):
            eng.pmp_vjp(U, context_grad=True)
        torch.cuda.synchronize()
        return
    for _ in range(2):
        eng.pmp_vjp(U); eng.pmp_vjp(U, context_grad=True)
    plain, with_g = [], []
    for _ in range(7):
        plain.append(timed(lambda: eng.pmp_vjp(U)))
        with_g.append(timed(lambda: eng.pmp_vjp(U, context_grad=True)))
    # one inner iteration of NullTextInversion.run on one engine (eps_C given)
    eps_c, target = torch.randn_like(z), torch.randn_like(z)
    null.grad = torch.zeros_like(null)
    opt = torch.optim.Adam([null], lr=1e-2)
    w, n = 7.5, z.numel()
    gscale = (1.0 - w) * eps_coefficient(at, at_next) * 2.0 / n

    def inner():
        eng.set_context(null)
        eng.pmp_primal(z, t, at, None, use_et=True)
        eps_n = eng.pmp_primal_eps().view_as(z)
        z_prev, _ = eng.sched_step(z, eng.lincomb([(w, eps_c), (1.0 - w, eps_n)]), at, at_next)
        diff = z_prev - target
        loss = (diff * diff).mean()
        _, G = eng.pmp_vjp((gscale * diff).reshape(1, n).contiguous(), context_grad=True)
        null.grad.copy_(G[0])
        opt.step()
        return float(loss)
    for _ in range(2):
        inner()
    it = [timed(inner) for _ in range(7)]
    fwd = [timed(lambda: eng.unet_forward(z, t)) for _ in range(9)][2:]
    src = torch.empty(256 << 20, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    cp = [timed(lambda: dst.copy_(src)) for _ in range(7)]
    rate = 2 * src.numel() * 4 / (statistics.median(cp) * 1e-3) / 1e12      # TB/s, read + write
    lines = ["| part | ms (median of 7) | min - max |", "|---|---|---|",
             f"| pmp_vjp, k = 1 | {stats(plain)} |", f"| pmp_vjp(context_grad=True), k = 1 | {stats(with_g)} |",
             f"| unet_forward, B = 1 | {stats(fwd)} |", f"| one inner iteration of null-text inversion | {stats(it)} |",
             "", f"device-to-device copy of 1 GiB: {statistics.median(cp):.3f} ms = {rate:.2f} TB/s (read + write)", "",
             "| level: tokens x channels | stages | MB per stage (q, g_o, P read once; partials written and read) | us per stage at the copy rate |",
             "|---|---|---|---|"]
    for T, C, nst, b in stage_bytes(cfg):
        lines.append(f"| {T} x {C} | {nst} | {b / 1e6:.2f} | {b / (rate * 1e12) * 1e6:.1f} |")
    text = "\n".join(lines)
    print(text)
    if outp:
        os.makedirs(os.path.dirname(os.path.abspath(outp)), exist_ok=True)
        with open(outp, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
