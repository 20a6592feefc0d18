"""Time per power iteration of the three Jacobian targets, and of the h-space forwards, on CELEBA_DDPM at 256 x 256.

    python tests/diag/hspace_time.py [out.md]

One process, one GPU, bf16x3, k = 5 probes, two streams: ms per power iteration (one batched J V, one batched J^T U, the
re-orthonormalisation) of the x0 target (the unchanged path: the comparison), of h_enc (d h / d x_t) and of h_dec (d eps / d h),
interleaved, three runs each; then ms of get_h and forward_dh against unet_forward at B = 5.  Each tap pass launches a strict
subset of the full pass's convs, so h_enc <= x0 and h_dec <= x0 is the expectation this measures.  Writes a markdown table
(default: stdout only)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import solver  # noqa: E402
from loco_edit_amd.config import CELEBA_DDPM, synth_params  # noqa: E402
from loco_edit_amd.hip import LocoEngine  # noqa: E402

K, ITERS, RUNS, T, AT = 5, 4, 3, 601.0, 0.0253


def main():
    dev = torch.device("cuda:0")
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=8, device=dev)
    eng.load_state_dict(synth_params(cfg, 0))
    eng.set_precision("bf16x3")
    n_streams = eng.set_streams_measured(2)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 3, cfg.resolution, cfg.resolution, generator=g).to(dev)
    mask = torch.zeros(3, cfg.resolution, cfg.resolution, dtype=torch.bool)
    mask[:, 96:160, 80:176] = True
    mask = mask.to(dev)
    widths = {"x0": eng.n, "h_enc": eng.n, "h_dec": eng.n_h}
    v0 = {tg: torch.randn(n, K, generator=g).to(dev) for tg, n in widths.items()}

    def solve(target, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.local_basis(eng, x, T, AT, K, mask=None if target == "h_enc" else mask, noise=(target != "x0"), min_iter=iters,
                           max_iter=iters, v0=v0[target], verbose=False, solver="power", target=target)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for tg in widths:                            # warm-up: lazy set-up of every launcher on every path
        solve(tg, 2)
    per_iter = {tg: [] for tg in widths}
    for _ in range(RUNS):
        for tg in widths:                        # interleaved; the primal and the QR of V0 cancel in the difference of two solves
            per_iter[tg].append((solve(tg, ITERS + 2) - solve(tg, 2)) / ITERS * 1e3)

    xb = torch.randn(5, 3, cfg.resolution, cfg.resolution, generator=g).to(dev)
    dh = torch.randn(5, eng.n_h, generator=g).to(dev)
    fwd = {"unet_forward": lambda: eng.unet_forward(xb, T), "get_h": lambda: eng.get_h(xb, T),
           "forward_dh": lambda: eng.unet_forward(xb, T, dh=dh)}
    fwd_ms = {n: [] for n in fwd}
    for f in fwd.values():
        f()
    for _ in range(RUNS):
        for n, f in fwd.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                f()
            torch.cuda.synchronize()
            fwd_ms[n].append((time.perf_counter() - t0) / 5 * 1e3)

    lines = [f"CELEBA_DDPM 256 x 256, bf16x3, k = {K}, streams = {n_streams}, n_h = {eng.n_h} {eng.h_shape}; three interleaved runs",
             "", "| target | ms per power iteration (runs) | median |", "|---|---|---|"]
    med = lambda v: sorted(v)[len(v) // 2]
    for tg, v in per_iter.items():
        lines.append(f"| {tg} | {', '.join(f'{a:.2f}' for a in v)} | {med(v):.2f} |")
    lines += ["", "| B = 5 | ms (runs) | median |", "|---|---|---|"]
    for n, v in fwd_ms.items():
        lines.append(f"| {n} | {', '.join(f'{a:.2f}' for a in v)} | {med(v):.2f} |")
    ok = med(per_iter["h_enc"]) <= med(per_iter["x0"]) and med(per_iter["h_dec"]) <= med(per_iter["x0"])
    lines += ["", f"h_enc <= x0 and h_dec <= x0 per iteration: {'holds' if ok else 'FAILS'}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
