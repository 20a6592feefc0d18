#!/usr/bin/env python3
"""Block Krylov solver next to the block power iteration on the headline configuration (bench.py's x / t / mask / V0,
CelebA-HQ DDPM architecture at 256 x 256 with the synthetic checkpoint, 5 + 5 probes: the modify-space and null-space
solves sharing one batch per pass as in ``solver.local_basis_pair``).  A diagnostic, not a test; not part of bench.py.

Reports (JSON on stdout and, with --out, into a file):
  (a) ms per Krylov step at every basis size (5 + 5 ... 60 + 60 rows) and ms per power iteration: same process, the two
      solvers interleaved, ``--runs`` runs each (device events around every step; each step ends in its readback)
  (b) the share of a step spent in the solver's own algebra (everything but the J V and J^T U passes)
  (c) steps against accuracy for both solvers: smallest principal cosine of each solve's span against a 50-iteration
      power basis, and the Krylov solver's residual estimates
and the average shader clock over the timed part.

    python tests/diag/solver_compare.py [--runs 3] [--steps 12] [--precision bf16x3] [--out profiles/<name>.json]
    rocprofv3 --kernel-trace --stats -d <dir> -o s --output-format csv -- python tests/diag/solver_compare.py --only-krylov
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch      # noqa: E402

import bench      # noqa: E402
import loco_edit_amd  # noqa: F401,E402
from loco_edit_amd import solver      # noqa: E402
from loco_edit_amd.config import CELEBA_DDPM, synth_params      # noqa: E402
from loco_edit_amd.hip import LocoEngine      # noqa: E402
from loco_edit_amd.scheduler import YHCustomScheduler      # noqa: E402


def principal_cos(Va, Vb):
    qa = torch.linalg.qr(Va.detach().cpu().double().T)[0]
    qb = torch.linalg.qr(Vb.detach().cpu().double().T)[0]
    return torch.linalg.svdvals(qa.T @ qb).min().item()


class Timer:
    """Device events at the marks of one step: start, after the two passes, after the algebra (and its readback)."""

    def __init__(self):
        self.rows = []

    def step(self, passes, algebra):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = passes()
        e[1].record()
        res = algebra(*out)
        e[2].record()
        e[2].synchronize()
        self.rows.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))
        return res


def start_blocks(eng, v0s):
    V = [v.T.contiguous() for v in v0s]
    for v in V:
        eng.qr_rows_(v)
    return V


def krylov_pair(eng, x, t, at, masks, v0s, steps, keep=False):
    """``solver._krylov_pair`` with both solves kept running for ``steps`` steps (no exit but the row limit), timed per
    step.  -> (timer rows, per step [(Y_a, resid_a), (Y_b, resid_b)] when ``keep``)."""
    V = start_blocks(eng, v0s)
    st = [solver.KrylovState(eng, V[j], eng.n_out, (0, V[j].shape[0]), slot=j) for j in (0, 1)]
    op = solver.JacobianOperator(eng, x, t, at, masks[0], False)
    ka = V[0].shape[0]
    eng.pmp_set_second_mask(masks[1].to(torch.uint8).contiguous().view(-1), ka)
    tm, hist = Timer(), []
    for i in range(steps):
        def passes():
            U = op.jvp(torch.cat([s.block() for s in st]))
            return U, op.vjp(U)

        def algebra(U, A):
            return [st[0].advance(U[:ka], A[:ka], -1.0, last=(i == steps - 1)), st[1].advance(U[ka:], A[ka:], -1.0, last=(i == steps - 1))]
        done = tm.step(passes, algebra)
        if keep:
            hist.append([(s.Y[(s.steps - 1) % 2].clone(), s.resid.tolist()) for s in st])
        if any(done):
            break
    eng.pmp_set_second_mask(None)
    return tm.rows, hist


def power_pair(eng, x, t, at, masks, v0s, iters):
    """The power loop of ``solver.local_basis_pair`` (both solves for ``iters`` iterations), timed per iteration."""
    V = start_blocks(eng, v0s)
    op = solver.JacobianOperator(eng, x, t, at, masks[0], False)
    ka = V[0].shape[0]
    eng.pmp_set_second_mask(masks[1].to(torch.uint8).contiguous().view(-1), ka)
    tm = Timer()
    for _ in range(iters):
        def passes():
            U = op.jvp(torch.cat(V))
            return U, op.vjp(U)

        def algebra(U, A):
            out = [A[:ka].contiguous(), A[ka:].contiguous()]
            for j in (0, 1):
                eng.orthonormalize_(out[j])
            torch.cuda.synchronize()
            return out
        V = tm.step(passes, algebra)
    eng.pmp_set_second_mask(None)
    return tm.rows, V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["f32", "bf16x3", "f16"])
    ap.add_argument("--out", default="")
    ap.add_argument("--only-krylov", action="store_true",
                    help="warm up, run one Krylov pair of --steps steps and stop: the run to put under a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = CELEBA_DDPM
    eng = LocoEngine(cfg, max_batch=32, device=dev)
    eng.load_state_dict(synth_params(cfg, seed=0))
    eng.set_precision(a.precision)
    eng.set_streams_measured(2)
    sched = YHCustomScheduler()
    sched.set_timesteps(100)
    t = float(sched.timesteps[40])
    at = sched.alpha_at(t)
    x, mask, v0 = bench.synthetic_inputs(cfg, 10, dev)
    masks, v0s = (mask, ~mask), (v0[:, :5].contiguous(), v0[:, 5:].contiguous())

    # warm-up of every shape both loops use, then the accuracy reference: 50 power iterations
    krylov_pair(eng, x, t, at, masks, v0s, 2)
    if a.only_krylov:
        rows, _ = krylov_pair(eng, x, t, at, masks, v0s, a.steps)
        print(json.dumps({"ms_passes": [round(r[0], 3) for r in rows], "ms_algebra": [round(r[1], 3) for r in rows]}))
        return
    power_pair(eng, x, t, at, masks, v0s, 2)
    _, ref = power_pair(eng, x, t, at, masks, v0s, 50)

    ck0 = eng.clock_stamp()
    k_runs, p_runs = [], []
    for _ in range(a.runs):                       # interleaved
        k_runs.append(krylov_pair(eng, x, t, at, masks, v0s, a.steps)[0])
        p_runs.append(power_pair(eng, x, t, at, masks, v0s, a.steps)[0])
    ck1 = eng.clock_stamp()
    torch.cuda.synchronize()

    # (c) accuracy per step
    _, hist = krylov_pair(eng, x, t, at, masks, v0s, a.steps, keep=True)
    acc = []
    for j in range(1, a.steps + 1):
        row = {"steps": j}
        if j <= len(hist):
            row["krylov_cos"] = [principal_cos(hist[j - 1][s][0], ref[s]) for s in (0, 1)]
            row["krylov_resid_max"] = [max(hist[j - 1][s][1]) for s in (0, 1)]
        if j % 2 == 0 or j == 1:
            _, Vp = power_pair(eng, x, t, at, masks, v0s, j)
            row["power_cos"] = [principal_cos(Vp[s], ref[s]) for s in (0, 1)]
        acc.append(row)

    def med(v):
        v = sorted(v)
        return v[len(v) // 2]
    n_k = min(len(r) for r in k_runs)
    steps = []
    for j in range(n_k):
        pas, alg = [r[j][0] for r in k_runs], [r[j][1] for r in k_runs]
        steps.append({"rows_per_solve": 5 * (j + 1), "ms_passes": [round(v, 3) for v in pas], "ms_algebra": [round(v, 3) for v in alg],
                      "ms_step_median": round(med([p + q for p, q in zip(pas, alg)]), 3),
                      "algebra_share_median": round(med([q / (p + q) for p, q in zip(pas, alg)]), 4)})
    p_pas = [v[0] for r in p_runs for v in r]
    p_alg = [v[1] for r in p_runs for v in r]
    out = {
        "config": {"model": "CELEBA_DDPM synthetic seed 0", "precision": a.precision, "probes": "5 + 5 (local_basis_pair)",
                   "runs": a.runs, "steps": a.steps},
        "clock": {"sclk_mhz_avg_over_timed_region": round(LocoEngine.sclk_mhz(ck0, ck1), 1)},
        "krylov_steps": steps,
        "power_iteration": {"ms_passes_median": round(med(p_pas), 3), "ms_algebra_median": round(med(p_alg), 3),
                            "ms_iteration_median": round(med([p + q for p, q in zip(p_pas, p_alg)]), 3),
                            "ms_iteration_min_max": [round(min(p + q for p, q in zip(p_pas, p_alg)), 3),
                                                     round(max(p + q for p, q in zip(p_pas, p_alg)), 3)]},
        "accuracy_vs_power_50": acc,
    }
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
