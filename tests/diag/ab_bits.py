"""Diagnostic (by hand): bit-for-bit A/B of every library under tests/diag/lib on one box (LOCO_HIP_LIB) -- the check behind a
host-side change of the passes, which must leave every launch and every argument alone.

Each library runs in a fresh child process under its own time limit: the tiny configurations (every op kind, all three `updown`
values, has_nin, scale_shift, added_kv, has_x, XFMR, ksize == 1) x the three conv arithmetics x forward, forward with a dh,
primal + J V + J^T U for 2 probes (one lane) and 5 (two lanes), and the encoder / decoder taps where the network has a
bottleneck.  Seeded weights and inputs.  A child prints one line per output with its sha256 and, per configuration and
arithmetic, from a second, profiled run of the same operations (a profiled pass keeps its probes on one lane), the outputs'
hashes again and the conv profile in shape mode without its time column (kernel, shape key, launches, flops).  The parent stops at the
first child that does not exit 0 and exits non-zero if any two libraries differ on any line.

    python tests/diag/ab_bits.py            # AB_BITS_TIMEOUT=<seconds per library>, default 600
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIBDIR = os.path.join(ROOT, "tests/diag/lib")
CONFIGS = ["TINY_DDPM", "TINY_ADM", "TINY_ADM_PLAIN", "TINY_ADM_XATTN", "TINY_LATENT_XATTN", "TINY_LDM", "TINY_IF", "TINY_ENCODER",
           "TINY_DECODER"]
PRECS = ["f32", "bf16x3", "f16"]
T, AT = 601.0, 0.37


def child():
    sys.path.insert(0, ROOT)
    import torch
    import loco_edit_amd  # noqa: F401
    from loco_edit_amd import config as K
    from loco_edit_amd.hip import LocoEngine
    dev = torch.device("cuda:0")

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    for name in CONFIGS:
        cfg = getattr(K, name)
        g = torch.Generator().manual_seed(7)
        rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)      # noqa: E731
        eng = LocoEngine(cfg, max_batch=8, device=dev)
        eng.load_state_dict(K.synth_params(cfg, 0))
        if cfg.context_dim:
            eng.set_context(rnd(cfg.context_len, cfg.context_dim))
        if cfg.added_kv:
            eng.set_cond(rnd(4 * cfg.ch))
        eng.set_streams(2)                     # 4 probes and more: two lanes
        try:
            n_h = eng.n_h
        except RuntimeError:                   # the latent decoder / encoder: no bottleneck
            n_h = 0
        R, Ro = cfg.resolution, cfg.out_resolution
        xs = rnd(5, cfg.in_channels, R, R)
        x1 = xs[:1].contiguous()
        mask = torch.zeros(cfg.out_ch, Ro, Ro, dtype=torch.bool)
        mask[:, Ro // 3:Ro // 2 + 1, Ro // 4:Ro // 2 + 1] = True
        mask = mask.to(dev)
        V, U = rnd(5, eng.n), rnd(5, eng.n_out)
        dh, Vh, Uh = (rnd(5, n_h), rnd(5, n_h), rnd(5, n_h)) if n_h else (None, None, None)
        use_et = eng.n_out != eng.n

        def run_ops():
            out = {"fwd1": eng.unet_forward(x1, T), "fwd5": eng.unet_forward(xs, T)}
            if n_h:
                out["fwd5_dh"] = eng.unet_forward(xs, T, dh=dh)
            eng.pmp_primal(x1, T, AT, mask, use_et=use_et)
            for k in (2, 5):
                out[f"jvp{k}"] = eng.pmp_jvp(V[:k].contiguous())
                out[f"vjp{k}"] = eng.pmp_vjp(U[:k].contiguous())
            if n_h:
                eng.pmp_primal(x1, T, AT, None, tap="enc")
                for k in (2, 5):
                    out[f"enc_jvp{k}"] = eng.pmp_jvp(V[:k].contiguous())
                    out[f"enc_vjp{k}"] = eng.pmp_vjp(Uh[:k].contiguous())
                eng.pmp_primal(x1, T, AT, mask, tap="dec")
                for k in (2, 5):
                    out[f"dec_jvp{k}"] = eng.pmp_jvp(Vh[:k].contiguous())
                    out[f"dec_vjp{k}"] = eng.pmp_vjp(U[:k].contiguous())
            return out

        for prec in PRECS:
            eng.set_precision(prec)
            for op, t in run_ops().items():      # profile off: 5 probes run as two lanes
                print(name, prec, op, sha(t), flush=True)
            eng.profile_enable(2)                # the launch list (a profiled pass runs its probes as one lane)
            for op, t in run_ops().items():
                print(name, prec, "profiled", op, sha(t), flush=True)
            for key, r in sorted(eng.profile_report().items()):
                print(name, prec, "launch", key, r["launches"], "%.6e" % r["flops"], flush=True)
            eng.profile_enable(False)
        del eng
        torch.cuda.empty_cache()


def main():
    libs = sorted(f for f in os.listdir(LIBDIR) if f.endswith(".so"))
    if len(libs) < 2:
        sys.exit(f"need at least two libraries under {LIBDIR}, found {libs}")
    limit = os.environ.get("AB_BITS_TIMEOUT", "600")
    lines = {}
    for l in libs:
        env = dict(os.environ, LOCO_HIP_LIB=os.path.join(LIBDIR, l))
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--child"], env=env,
                           capture_output=True, text=True)
        if r.returncode != 0:      # nothing more is started on the GPU after a child that failed
            print(r.stdout[-2000:], r.stderr[-2000:], sep="\n")
            sys.exit(f"{l}: child exited {r.returncode}")
        lines[l] = r.stdout.splitlines()
        print(f"{l}: {len(lines[l])} lines", flush=True)
    ref = libs[0]
    bad = 0
    for l in libs[1:]:
        if len(lines[l]) != len(lines[ref]):
            print(f"{l}: {len(lines[l])} lines, {ref}: {len(lines[ref])}")
            bad += 1
        for a, b in zip(lines[ref], lines[l]):
            if a != b:
                print(f"- {ref}: {a}\n+ {l}: {b}")
                bad += 1
    for a in lines[ref]:
        print(a)
    print(f"{len(libs)} libraries, {len(lines[ref])} lines each: " + ("IDENTICAL" if not bad else f"{bad} DIFFERENCES"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
