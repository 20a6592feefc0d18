"""CPU checks behind tests/test_gpu_norm_offsets.py: the oracle runs in float64 (no silent fp32 step), its fp32 results are
the same bits as before, and the offset weights of tests/norm_offsets.py reach the regime the GPU legs claim.

  - float64 oracle: a float64 forward / J V of every architecture the GPU module covers (DDPM, guided-diffusion ADM with and
    without scale-shift norm, latent decoder, latent-diffusion U-Net with SpatialTransformer) never produces an fp32 tensor
    from a float64 one, and agrees with the fp32 run to fp32 accuracy;
  - regime: max |mean| / std of the inputs of the norms fed by a conv >= 50 ("moderate") and >= 1000 ("severe");
  - hardness: the fp32 oracle's own rel-L2 against float64 grows >= 10x from no offset to "severe"."""
import pytest
import torch
from torch.overrides import TorchFunctionMode
from torch.utils._pytree import tree_flatten

import loco_oracle as orc
import norm_offsets as no
from loco_edit_amd.config import MID_DDPM, TINY_ADM, TINY_ADM_PLAIN, TINY_DDPM, TINY_DECODER, TINY_LDM

CFGS = {"tiny": TINY_DDPM, "mid": MID_DDPM, "tiny_adm": TINY_ADM, "tiny_decoder": TINY_DECODER, "tiny_ldm": TINY_LDM}


class _Downcasts(TorchFunctionMode):
    """Records every torch call that returns an fp32 tensor from a float64 argument (a `.float()`, `.to(float32)`, ...)."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if any(torch.is_tensor(a) and a.dtype == torch.float64 for a in tree_flatten((args, kwargs or {}))[0]):
            if any(torch.is_tensor(o) and o.dtype == torch.float32 for o in tree_flatten(out)[0]):
                self.seen.append(getattr(func, "__name__", str(func)))
        return out


@pytest.mark.parametrize("name,cfg", list(CFGS.items()) + [("tiny_adm_plain", TINY_ADM_PLAIN)])
def test_oracle_runs_in_float64(name, cfg):
    prm = no.offset_params(cfg, "zero")
    cs = no.case(cfg)
    p64 = no.to_torch(prm, torch.float64)
    f64 = no.operator(cfg, p64, cs)
    x = cs["x"].double()
    v = cs["V"][0].view_as(x).double()
    with _Downcasts() as mode:
        y, jv = torch.func.jvp(f64, (x,), (v,))
    assert not mode.seen, f"float64 oracle downcasts to fp32 in: {sorted(set(mode.seen))}"
    assert y.dtype == torch.float64 and jv.dtype == torch.float64
    f32 = no.operator(cfg, no.to_torch(prm), cs)
    y32, jv32 = torch.func.jvp(f32, (cs["x"],), (cs["V"][0].view_as(cs["x"]),))
    assert y32.dtype == torch.float32
    # an fp32 run is within fp32 accuracy of the float64 one, and not equal to it (the float64 run is not fp32 in disguise)
    assert 0 < no.rel(y32, y) < 1e-5 and 0 < no.rel(jv32, jv) < 1e-5


def test_timestep_embeddings_follow_the_requested_dtype():
    t = torch.tensor([603.0, 10.0])
    for fn in (orc.timestep_embedding, orc.timestep_embedding_adm):
        e32, e64 = fn(t, 33), fn(t, 33, torch.float64)
        assert e32.dtype == torch.float32 and e64.dtype == torch.float64
        assert torch.equal(fn(t, 33), fn(t.double(), 33)) and (e64 - e32.double()).abs().max() < 1e-4


@pytest.mark.parametrize("name", list(CFGS))
def test_offset_weights_reach_the_claimed_regime_and_make_fp32_lose_digits(name):
    cfg = CFGS[name]
    cs = no.case(cfg)
    worst = {}
    for level in ("moderate", "severe"):
        p64 = no.to_torch(no.offset_params(cfg, level), torch.float64)
        fed = no.conv_fed_norm_names(cfg, p64)
        with no.regime(p64) as seen, torch.no_grad():
            no.operator(cfg, p64, cs)(cs["x"].double())
        assert fed and fed <= set(seen), sorted(fed - set(seen))
        worst[level] = max(seen[k] for k in fed)
    zero = no.offset_params(cfg, "zero")
    assert all(zero[k] is v for k, v in no.synth_params(cfg, 0).items())      # level "zero" is synth_params itself
    err = {}
    for level in ("zero", "severe"):
        prm = no.offset_params(cfg, level)
        r64, r32 = no.reference(cfg, prm, cs, torch.float64), no.reference(cfg, prm, cs, torch.float32)
        err[level] = {k: no.rel(r32[k], r64[k]) for k in r64}
    print(f"{name}: max |mean|/std moderate {worst['moderate']:.0f}, severe {worst['severe']:.0f}; fp32 oracle vs float64 "
          + ", ".join(f"{k} {err['zero'][k]:.1e} -> {err['severe'][k]:.1e}" for k in err["zero"]))
    assert worst["moderate"] >= 50 and worst["severe"] >= 1000, worst
    assert err["severe"]["jv"] >= 10 * err["zero"]["jv"], err
