"""MI355X: the h-space PCA baselines (EditUncondDiffusion.inv_jac_xt / local_pca_xt / global_pca_xt, hspace_pca.decode_with_dh and
--run_edit_hspace_pca) on TINY_DDPM against what the reference's own functions computed (tests/golden/hspace_pca_tiny_ddpm*.pt,
written by tests/make_golden_hspace_pca.py), under f32 and bf16x3.

Bars are those of tests/test_gpu_hspace.py: get_h rel-L2 <= 2e-5 (f32) / 2e-4 (bf16x3); singular values rtol 1e-3; rows cos >= 0.999
(signed for inv_jac_xt: the reference's direction is the NEGATIVE normalised pullback).  With q = N - 1 the randomized PCA is the
exact SVD of the centred samples whatever the range finder drew, so the reference's result is comparable row by row where
``gap_rows`` says the singular value is >= 1 % away from its neighbours.
"""
import os
from argparse import Namespace

import pytest
import torch

import loco_oracle as orc
from loco_edit_amd.config import TINY_DDPM, synth_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECS = ["f32", "bf16x3"]
FWD = {"f32": 2e-5, "bf16x3": 2e-4}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 601.0


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


def cos_rows(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))


_FX = {}


def fx(name):
    if name not in _FX:
        _FX[name] = torch.load(os.path.join(GOLD, name + ".pt"))
    return _FX[name]


def new_engine(max_batch=4):
    from loco_edit_amd.hip import LocoEngine
    e = LocoEngine(TINY_DDPM, max_batch=max_batch, device=torch.device(DEV))
    e.load_state_dict(synth_params(TINY_DDPM, 0))
    return e


@pytest.fixture(scope="module")
def engine():
    return new_engine()


class _Sched:
    def __init__(self, at):
        self.at = at

    def alpha_at(self, t):
        return self.at


AT = float(orc.Scheduler().alpha_at(torch.tensor(int(T))))


def stub_edit(eng):
    """An EditUncondDiffusion around an existing engine (its constructor builds the model from CLI arguments)."""
    from loco_edit_amd.dist import ProbeSharder
    from loco_edit_amd.edit import EditUncondDiffusion
    ed = object.__new__(EditUncondDiffusion)
    ed.engine, ed.device, ed.scheduler, ed.sharder, ed.seed = eng, torch.device(DEV), _Sched(AT), ProbeSharder(None), 7
    return ed


# ------------------------------------------------------------------------------------------------------------ the samples
@pytest.mark.parametrize("prec", PRECS)
def test_sample_matrix_matches_the_reference(prec, engine):
    from loco_edit_amd import hspace_pca
    engine.set_precision(prec)
    g = fx("hspace_pca_tiny_ddpm")
    xs = g["x"].to(DEV) + hspace_pca.normalize_wrt_batch(g["noise"].to(DEV))
    store = hspace_pca.sample_h(engine, xs, T)
    H = store.centered(center=False)[0]
    print(f"{prec}: local sample matrix {rel(H, g['H']):.2e}")
    assert store.rows == 12 and rel(H, g["H"]) < FWD[prec]
    gg = fx("hspace_pca_tiny_ddpm_global")
    Hg = hspace_pca.sample_h(engine, gg["x"], T).centered(center=False)[0]
    print(f"{prec}: global sample matrix {rel(Hg, gg['H']):.2e}")
    assert rel(Hg, gg["H"]) < FWD[prec]


# ------------------------------------------------------------------------------------------------------------ inv_jac_xt
@pytest.mark.parametrize("prec", PRECS)
def test_inv_jac_xt(prec, engine):
    engine.set_precision(prec)
    g = fx("hspace_pca_tiny_ddpm")
    ed = stub_edit(engine)
    x, u = g["x"].to(DEV), g["u"].to(DEV)
    vT = ed.inv_jac_xt(x=x, t=T, op='mid', block_idx=0, u=u, perturb_h=0.1)
    assert tuple(vT.shape) == tuple(g["vT"].shape)
    cos = cos_rows(vT, g["vT"])
    print(f"{prec}: signed cos min {float(cos.min()):.7f}")
    assert float(cos.min()) >= 0.999                        # signed: -J^T u, not +
    assert torch.equal(ed.inv_jac_xt(x=x, t=T, op='mid', block_idx=0, u=u, perturb_h=1.0), vT)
    one = ed.inv_jac_xt(x=x, t=T, op='mid', block_idx=0, u=u[:, 2].contiguous())
    assert tuple(one.shape) == (1, vT.shape[1]) and float(cos_rows(one, vT[2:3])) >= 0.9999999
    assert float((vT.norm(dim=1) - 1).abs().max()) < 1e-5
    for op, bi in (("down", 0), ("mid", 1), ("up", 2)):
        with pytest.raises(NotImplementedError, match="only \\('mid', 0\\) is built"):
            ed.inv_jac_xt(x=x, t=T, op=op, block_idx=bi, u=u)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("prec", PRECS)
def test_local_pca_xt(prec, engine):
    engine.set_precision(prec)
    g = fx("hspace_pca_tiny_ddpm")
    ed = stub_edit(engine)
    kw = dict(x=g["x"].to(DEV), t=T, op='mid', block_idx=0, memory_bound=g["memory_bound"], num_pca_samples=12,
              pca_rank=g["pca_rank"], pca_device='cpu', perturb_h=g["perturb_h"], noise=g["noise"])
    u, s, vT = ed.local_pca_xt(return_x_direction=True, **kw)
    assert tuple(u.shape) == tuple(g["u"].shape) and tuple(s.shape) == tuple(g["s"].shape) and tuple(vT.shape) == tuple(g["vT"].shape)
    gap = g["gap_rows"]
    cu = cos_rows(u.T, g["u"].T)
    cv = cos_rows(vT, g["vT"]) * cu.sign()                     # the sign of a principal direction is a convention; vT follows u's
    print(f"{prec}: s rel {float(((s.cpu() - g['s']) / g['s']).abs().max()):.1e}, |cos u| min {float(cu.abs()[gap].min()):.6f}, "
          f"signed cos vT min {float(cv[gap].min()):.6f}")
    assert torch.allclose(s.cpu(), g["s"], rtol=1e-3)
    assert float(cu.abs()[gap].min()) >= 0.999 and float(cv[gap].min()) >= 0.999
    assert ed.last_pca["n_samples"] == 12 and tuple(ed.last_pca["mean"].shape) == (u.shape[0],)
    assert rel(ed.last_pca["mean"], g["H"].double().mean(dim=0)) < FWD[prec]
    u2, s2, none = ed.local_pca_xt(return_x_direction=False, **kw)
    assert none is None and torch.equal(u2, u) and torch.equal(s2, s)
    with pytest.raises(ValueError, match="noise must be"):
        ed.local_pca_xt(**dict(kw, noise=g["noise"][:5]))
    with pytest.raises(NotImplementedError):
        ed.local_pca_xt(**dict(kw, op='up'))
    # without injected noise: runs, and q beyond N - 1 is the unit's refusal
    u3, s3, _ = ed.local_pca_xt(**dict(kw, noise=None, num_pca_samples=6, pca_rank=3, return_x_direction=False))
    assert tuple(u3.shape) == (u.shape[0], 3) and bool(torch.isfinite(s3).all())
    with pytest.raises(RuntimeError, match=r"exceeds min\(N - 1, D\)"):
        ed.local_pca_xt(**dict(kw, noise=None, num_pca_samples=4, pca_rank=4, return_x_direction=False))


@pytest.mark.parametrize("prec", PRECS)
def test_global_pca_xt(prec, engine):
    engine.set_precision(prec)
    g = fx("hspace_pca_tiny_ddpm_global")
    ed = stub_edit(engine)
    u, s = ed.global_pca_xt(x=g["x"], t=T, op='mid', block_idx=0, memory_bound=g["memory_bound"], pca_rank=g["pca_rank"],
                            pca_device='cpu')
    assert tuple(u.shape) == tuple(g["u"].shape) and tuple(s.shape) == tuple(g["s"].shape)
    cu = cos_rows(u.T, g["u"].T).abs()[g["gap_rows"]]
    print(f"{prec}: s rel {float(((s.cpu() - g['s']) / g['s']).abs().max()):.1e}, |cos u| min over the gap rows {float(cu.min()):.6f}")
    assert torch.allclose(s.cpu(), g["s"], rtol=1e-3) and float(cu.min()) >= 0.999
    assert ed.last_pca["n_samples"] == 13


def test_state_hygiene_after_a_pca_run():
    """x0 products after a PCA run (partial forwards, an encoder primal, cotangent passes) are what a fresh context computes."""
    g = fx("hspace_pca_tiny_ddpm")
    gen = torch.Generator().manual_seed(4)
    x2 = torch.randn(1, 3, 32, 32, generator=gen).to(DEV)
    V, U = torch.randn(3, 3072, generator=gen).to(DEV), torch.randn(3, 3072, generator=gen).to(DEV)
    mask = torch.zeros(3, 32, 32, dtype=torch.bool)
    mask[:, 9:22, 5:19] = True

    def full(e):
        e.pmp_primal(x2, T, AT, mask.to(DEV))
        return e.pmp_jvp(V), e.pmp_vjp(U), e.unet_forward(x2, T)
    fresh = full(new_engine())
    e = new_engine()
    stub_edit(e).local_pca_xt(x=g["x"].to(DEV), t=T, op='mid', block_idx=0, num_pca_samples=12, pca_rank=5, noise=g["noise"])
    for a, b in zip(full(e), fresh):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the h walk
def make_edit(tmp_path, for_steps=20, pbt=0.0):
    os.environ.pop("WORLD_SIZE", None)
    from loco_edit_amd.edit import EditUncondDiffusion
    cfg = TINY_DDPM
    args = Namespace(device=torch.device(DEV), dtype=torch.float32, seed=1, model_name="tiny", unet_config=cfg,
                     synthetic_weights=0, ckpt_path="", max_batch=4, image_size=cfg.resolution, c_in=3,
                     dataset_name="Synthetic", dataset_root="", for_steps=for_steps, inv_steps=for_steps,
                     use_yh_custom_scheduler=True, edit_t=0.6, performance_boosting_t=pbt,
                     x_space_guidance_edit_step=1.0, x_space_guidance_scale=0.5, x_space_guidance_num_step=16,
                     result_folder=str(tmp_path), sample_idx=0, vT_path="", vT1_path="", choose_sem="l_eye", mask_index=0,
                     sampling_mode=False)
    return EditUncondDiffusion(args)


@pytest.mark.parametrize("prec", PRECS)
def test_h_walk(prec, tmp_path):
    from loco_edit_amd import hspace_pca
    ed = make_edit(tmp_path)
    ed.engine.set_precision(prec)
    g = fx("hspace_pca_tiny_ddpm")
    xt = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    alphas = [-8.0, -4.0, 0.0, 4.0, 8.0]                   # more frames than max_batch: two chunks
    sigma = float(g["s"][0]) / (12 - 1) ** 0.5
    dh = torch.tensor(alphas)[:, None] * sigma * g["u"][:, 0][None, :]
    batch = hspace_pca.decode_with_dh(ed, xt.expand(5, -1, -1, -1), ed.edit_t_idx, dh)
    plain = hspace_pca.decode_with_dh(ed, xt.expand(5, -1, -1, -1), ed.edit_t_idx, None)[2:3]
    assert tuple(batch.shape) == (5, 3, 32, 32) and bool(torch.isfinite(batch).all())
    assert torch.equal(batch[2:3], plain)                   # alpha = 0: the same loop without dh
    for j in (0, 1, 3, 4):
        assert not torch.equal(batch[j], batch[2])
    moved = [rel(batch[j:j + 1], plain) for j in range(5)]
    print(f"{prec}: frames moved by {[f'{m:.1e}' for m in moved]}")
    assert moved[0] > moved[1] > 0 and moved[4] > moved[3] > 0 and moved[2] == 0
    alone = hspace_pca.decode_with_dh(ed, xt, ed.edit_t_idx, dh[3:4])
    assert torch.equal(alone, batch[3:4])                   # a frame decoded alone is its row of the batch


# ------------------------------------------------------------------------------------------------------------ the driver
def driver_argv(kind, edit):
    return ["--sh_file_name", "main_celeba_hf_null_space_projection.sh", "--sample_idx", "3", "--device", DEV,
            "--dtype", "fp32", "--seed", "11", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Synthetic",
            "--unet_preset", "tiny_ddpm", "--synthetic_weights", "0", "--for_steps", "100", "--inv_steps", "100",
            "--use_yh_custom_scheduler", "True", "--x_space_guidance_edit_step", "1", "--x_space_guidance_scale", "0.5",
            "--x_space_guidance_num_step", "16", "--edit_t", "0.6", "--performance_boosting_t", "0.2",
            "--choose_sem", "l_eye", "--use_mask", "True", "--pca_rank", "2", "--vis_num", "2", "--max_batch", "8",
            "--run_edit_hspace_pca", "True", "--hspace_pca", kind, "--hspace_pca_samples", "12", "--hspace_pca_rank", "4",
            "--hspace_edit", edit]


@pytest.mark.parametrize("edit", ["h", "x"])
@pytest.mark.parametrize("kind", ["global", "local"])
def test_driver(kind, edit, tmp_path, monkeypatch):
    from loco_edit_amd import hspace_pca
    from loco_edit_amd.main import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("LOCO_PRECISION", "bf16x3")
    out = main(driver_argv(kind, edit))
    assert tuple(out.shape) == (10, 3, 32, 32) and bool(torch.isfinite(out).all())
    rdir = tmp_path / "runs" / "CelebA_HQ_HF-Synthetic" / "results" / "sample_idx3"
    bpath = rdir / "basis" / "hspace_pca-0.6T" / f"hspace-pca-{kind}-rank-4-samples-12.pt"
    basis = torch.load(bpath)
    assert sorted(basis) == ["kind", "mean", "n_samples", "s", "t", "u"]
    assert tuple(basis["u"].shape) == (4096, 4) and tuple(basis["s"].shape) == (4,) and tuple(basis["mean"].shape) == (4096,)
    assert basis["kind"] == kind and basis["n_samples"] == 12 and bool((basis["s"][:-1] >= basis["s"][1:]).all())
    assert float((basis["u"].T @ basis["u"] - torch.eye(4)).abs().max()) < 1e-4
    grids = sorted(f for f in os.listdir(rdir) if f.startswith("3-Edit-hspace_pca-") and f.endswith(".png"))
    assert len(grids) == 2 and all(f"-{kind}-" in f and f"T-{edit}-rank4" in f for f in grids)
    assert not torch.equal(out[0], out[2]) and not torch.equal(out[4], out[2])      # the walk moves the image, both ways

    # a second run takes the basis from the file: no sample is drawn
    def no_sampling(*a, **k):
        raise AssertionError("the basis file was not reused")
    monkeypatch.setattr(hspace_pca, "sample_h", no_sampling)
    again = main(driver_argv(kind, edit))
    assert torch.equal(again, out)


def test_driver_refusals():
    from loco_edit_amd.define_argparser import parse_args
    ok = driver_argv("global", "h")
    parse_args(ok)

    def swap(flag, val):
        a = list(ok)
        a[a.index(flag) + 1] = val
        return a
    with pytest.raises(ValueError, match="built for the unconditional models"):
        parse_args(swap("--model_name", "stable-diffusion-v1-5"))
    with pytest.raises(ValueError, match="built for the unconditional models"):
        parse_args(swap("--model_name", "DeepFloyd/IF-I-M-v1.0"))
    with pytest.raises(ValueError, match=r"--hspace_pca_rank 12 must lie in \[1, min\(samples - 1, 512\)\] = \[1, 11\]"):
        parse_args(swap("--hspace_pca_rank", "12"))
    with pytest.raises(ValueError, match="at least 3 samples"):
        parse_args(swap("--hspace_pca_samples", "2"))
    with pytest.raises(ValueError, match="--pca_rank 5 directions are shown"):
        parse_args(swap("--pca_rank", "5"))
    with pytest.raises(ValueError, match="scales the h-space walk"):
        parse_args(swap("--hspace_edit", "x") + ["--hspace_edit_scale", "2"])
    with pytest.raises(ValueError, match="must be positive"):
        parse_args(ok + ["--hspace_edit_scale", "0"])
    with pytest.raises(ValueError, match="--vT_path"):
        parse_args(ok + ["--vT_path", "some.pt"])
    with pytest.raises(ValueError, match="--hspace_pca_samples is read by --run_edit_hspace_pca only"):
        parse_args(swap("--run_edit_hspace_pca", "False") + ["--run_edit_null_space_projection", "True"])
    with pytest.raises(SystemExit):
        parse_args(swap("--hspace_pca", "both"))
