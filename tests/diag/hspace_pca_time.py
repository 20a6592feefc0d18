"""Time of the h-space PCA baselines on CELEBA_DDPM at 256 x 256 (n_h = 32 768): sampling, and the device PCA phase by phase.

    python tests/diag/hspace_pca_time.py [out.md] [--big] [--cpu]

One process, one GPU, bf16x3.  Sampling: 1000 rows of get_h, max_batch at a time, appended to the store.  PCA at (N, q) =
(1000, 50), (10 000, 50) and with --big (50 000, 512), on a Gaussian sample matrix with a decaying column scale (the phases'
time does not depend on the values): centring, Hc W, Hc^T Q, the two Gram matrices, each called on its own through the
handle, and a whole fit at niter = 2; `rest` is what the fit spends beyond its 6 large products, 5 x 2 Grams and the centring
(the factor applications, the host algebra with its read-backs, the final product and the sign pass).  --cpu: torch.pca_lowrank
of the same matrix on the host's cores (the reference's pca_device='cpu' route), threads as the environment sets them.
Writes a markdown table (default: stdout only)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import hspace_pca  # noqa: E402
from loco_edit_amd.config import CELEBA_DDPM, synth_params  # noqa: E402
from loco_edit_amd.hip import LocoEngine, LocoPca  # noqa: E402

T, NITER = 601.0, 2
DEV = torch.device("cuda:0")


def timed(fn, reps=3):
    """Median ms of `fn` over `reps` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def sampling(lines):
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=8, device=DEV)
    eng.load_state_dict(synth_params(cfg, 0))
    eng.set_precision("bf16x3")
    xs = torch.randn(1000, 3, cfg.resolution, cfg.resolution, generator=torch.Generator().manual_seed(1))
    xs = xs.to(DEV)
    store = LocoPca(1000, eng.n_h, 50, device=DEV)

    def run():
        store.reset()
        hspace_pca.sample_h(eng, xs, T, store)
    ms = timed(run, reps=2)
    lines.append(f"sampling: 1000 rows of get_h (max_batch 8, bf16x3) into the store: {ms:.0f} ms ({ms / 1000:.2f} ms per row)")
    lines.append("")
    return eng.n_h


def pca(lines, D, N, q, cpu):
    g = torch.Generator(device="cuda").manual_seed(N)
    st = LocoPca(N, D, q, device=DEV)
    scale = (1.0 / (1.0 + torch.arange(D, device=DEV) / 64.0)).sqrt()
    for r0 in range(0, N, 2000):
        st.add_rows(torch.randn(min(2000, N - r0), D, generator=g, device=DEV) * scale + 0.5)
    omega = torch.randn(D, q, generator=g, device=DEV)
    Yn = torch.randn(N, q, generator=g, device=DEV)
    Yd = torch.randn(D, q, generator=g, device=DEV)

    def centre():
        st.center(False)                               # the other mode invalidates the cached centring: a copy of the store
        st.center(True)                                # column sums, means, the centred copy
    t_centre = timed(centre) / 2                       # mean of the two passes
    t_hw = timed(lambda: st.project(omega))
    r_hw = st.routes()
    t_htq = timed(lambda: st.project(Yn, transpose=True))
    r_htq = st.routes()
    t_gn = timed(lambda: st.gram(Yn))
    t_gd = timed(lambda: st.gram(Yd))
    t_fit = timed(lambda: st.fit(q, NITER, omega), reps=1 if q > 100 else 3)
    n_hw, n_htq = NITER + 1, NITER + 1
    rest = t_fit - n_hw * t_hw - n_htq * t_htq - 2 * (NITER + 1) * t_gn - 2 * NITER * t_gd - t_gd
    row = (f"| ({N}, {q}) | {t_centre:.1f} | {t_hw:.1f} ({r_hw.split(':')[1]}) | {t_htq:.1f} ({r_htq.split(':')[1]}) | {t_gn:.2f} / {t_gd:.2f} | "
           f"{rest:.0f} | {t_fit:.0f} |")
    if cpu:
        H = st.centered(center=False)[0].cpu()
        t0 = time.perf_counter()
        torch.pca_lowrank(H, q=q, center=True, niter=NITER)
        row += f" {(time.perf_counter() - t0) * 1e3:.0f} ({torch.get_num_threads()} threads) |"
    else:
        row += " not run |"
    lines.append(row)
    print(row, flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    big, cpu = "--big" in sys.argv, "--cpu" in sys.argv
    lines = []
    D = sampling(lines)
    print(lines[0], flush=True)
    lines.append(f"fit at niter = {NITER}, D = {D}; ms, medians of 3 (one run for q > 100); the fit centres once more only when the store changed")
    lines.append("")
    lines.append("| (N, q) | centring | Hc W (route) | Hc^T Q (route) | Gram over N / over D | rest | fit | torch.pca_lowrank on the host |")
    lines.append("|---|---|---|---|---|---|---|---|")
    for N, q in [(1000, 50), (10000, 50)] + ([(50000, 512)] if big else []):
        pca(lines, D, N, q, cpu and q <= 100)
    text = "\n".join(lines)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
