"""CPU: the host side of null-text inversion (loco_edit_amd.null_text, define_argparser, tloco_sd): the flags and their
defaults, the inv_steps / for_steps requirement, the published learning-rate schedule and stopping rule, the step coefficient
the gradient seed takes from the scheduler's formula, the cache file's round trip and the report, and -- a check of the GPU
test's own inputs -- that the float64 restatement of the optimiser is in the regime tests/test_gpu_null_text.py asserts in."""
import json
import math
import os

import pytest
import torch

import loco_edit_amd  # noqa: F401
from loco_edit_amd import define_argparser, null_text as nt


def test_flags_and_defaults():
    p = define_argparser.build_parser()
    a = p.parse_args([])
    assert a.null_text_inversion is False and a.null_text_inner_steps == 10
    assert a.null_text_lr == 1e-2 and a.null_text_early_stop == 1e-5
    a = p.parse_args(["--null_text_inversion", "True", "--null_text_inner_steps", "3", "--null_text_lr", "0.02",
                      "--null_text_early_stop", "1e-4"])
    assert a.null_text_inversion is True and a.null_text_inner_steps == 3
    assert a.null_text_lr == 0.02 and a.null_text_early_stop == 1e-4


def test_inv_steps_must_equal_for_steps():
    nt.check_steps(100, 100)
    with pytest.raises(ValueError, match="inv_steps == for_steps"):
        nt.check_steps(50, 100)
    try:
        nt.check_steps(50, 100)
    except ValueError as e:
        assert "inv_steps 50" in str(e) and "for_steps 100" in str(e)


def test_pmp_vjp_context_is_declared_and_bound():
    """The new entry point is in the header, in the symbol list build() checks, and in the Makefile's sources."""
    from loco_edit_amd.hip import SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "loco_pmp_vjp_context" in SYMBOLS
    assert "int  loco_pmp_vjp_context(loco_ctx* ctx, const float* U, int32_t k, float* A, float* G, void* stream);" in \
        open(os.path.join(root, "include", "loco_hip.h")).read()
    assert "xattn_ctx.hip" in open(os.path.join(root, "loco-edit_amd", "csrc", "Makefile")).read()


def test_lr_schedule_and_early_stop_rule():
    assert nt.step_lr(1e-2, 0) == 1e-2 and nt.step_lr(1e-2, 50) == pytest.approx(5e-3) and nt.step_lr(1e-2, 100) == 0.0
    assert nt.step_lr(2e-2, 25) == pytest.approx(1.5e-2)
    assert nt.stops_early(0.9e-5, 1e-5, 0) and not nt.stops_early(1.1e-5, 1e-5, 0)
    assert nt.stops_early(2.0e-4, 1e-5, 10) and not nt.stops_early(2.2e-4, 1e-5, 10)      # 1e-5 + 2e-5 * 10 = 2.1e-4


@pytest.mark.parametrize("at,at_next", [(0.5, 0.6), (0.0047, 0.0052), (0.98, 0.9991)])
def test_eps_coefficient_is_the_derivative_of_the_ddim_step(at, at_next):
    step = lambda e: math.sqrt(at_next) * (0.3 - math.sqrt(1 - at) * e) / math.sqrt(at) + math.sqrt(1 - at_next) * e
    d = step(1.0) - step(0.0)                                  # affine in eps
    # fp32 arithmetic, as loco_sched_step's: a difference of two terms of size <= 1, each a few roundings of 2^-24 relative
    assert nt.eps_coefficient(at, at_next) == pytest.approx(d, abs=8 * 2.0 ** -24 * 2)


def test_cache_round_trip_and_report(tmp_path):
    path = nt.cache_path(str(tmp_path), 3)
    assert path.endswith("null_text-3.pt") and nt.load_cache(path, 5, (7, 16)) is None
    g = torch.Generator().manual_seed(0)
    embs, zT = torch.randn(5, 7, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    report = {"steps": 5, "per_step": [{"first_loss": 0.5, "last_loss": 0.25, "inner_steps_used": 2, "seconds": 0.01}]}
    nt.save_cache(path, embs, zT, report)
    c = nt.load_cache(path, 5, (7, 16))
    assert torch.equal(c["embs"], embs) and torch.equal(c["zT"], zT) and c["report"] == report
    assert nt.load_cache(path, 6, (7, 16)) is None and nt.load_cache(path, 5, (77, 16)) is None     # another run length / context
    # ... and the settings and the image the cache was written for
    sha = nt.image_digest(zT)
    assert sha == nt.image_digest(zT.clone()) and sha != nt.image_digest(zT + 1e-3) and len(sha) == 64
    full = dict(report, inner_steps=2, lr=1e-2, early_stop=1e-5, guidance_scale=7.5, image_sha256=sha)
    nt.save_cache(path, embs, zT, full)
    ok = {"inner_steps": 2, "lr": 1e-2, "early_stop": 1e-5, "guidance_scale": 7.5, "image_sha256": sha}
    assert nt.load_cache(path, 5, (7, 16), ok) is not None
    for k, v in (("inner_steps", 3), ("lr", 2e-2), ("early_stop", 1e-4), ("guidance_scale", 5.0), ("image_sha256", nt.image_digest(zT * 2))):
        assert nt.load_cache(path, 5, (7, 16), dict(ok, **{k: v})) is None, k
    jp = os.path.join(str(tmp_path), "exp_null_text.json")
    nt.write_report(jp, report)
    assert json.load(open(jp)) == report


def test_the_optimiser_refuses_what_it_cannot_correct():
    from argparse import Namespace
    both = {"for": None, "edit": None, "null": None}
    with pytest.raises(ValueError, match="context_dim"):
        nt.NullTextInversion(Namespace(use_context=False, guidance_scale=7.5, branches=both))
    with pytest.raises(ValueError, match="guidance_scale"):
        nt.NullTextInversion(Namespace(use_context=True, guidance_scale=1.0, branches=both))
    with pytest.raises(ValueError, match="no null branch"):          # the latent-consistency class: for / edit only
        nt.NullTextInversion(Namespace(use_context=True, guidance_scale=7.5, branches={"for": None, "edit": None}))
    assert nt.NullTextInversion(Namespace(use_context=True, guidance_scale=7.5, branches=both)).seconds == []


def test_the_float64_restatement_is_in_the_regime_the_gpu_test_asserts():
    """tests/test_gpu_null_text.py compares Adam iterates, whose first steps are sign-like: no gradient entry of the float64 run
    may lie below 1e-6 of the largest; and it asserts that each outer step's last loss is at most its first, which the float64
    run itself must show for the seed and learning rate chosen."""
    import null_text_case as case
    c = case.build()
    for g in c["grads64"]:
        assert float(g.abs().min() / g.abs().max()) > 1e-6
    for li in c["losses64"]:
        assert len(li) == case.INNER and li[-1] <= li[0]
