"""CPU: the DiffEdit restatement (oracle/diffedit_oracle.py) against the fixture the reference's own
EditDeepFloydIF.mask_diffedit / MaskedDDPMforwardsteps produced (tests/golden/tloco_diffedit.pt,
oracle/make_golden_tloco_diffedit.py), the two threshold rules on hand-made maps, and the host logic of the product
module that needs no GPU."""
import pytest
import torch

import diffedit_oracle as do
import loco_oracle as orc
import tloco_oracle as tl
import loco_edit_amd  # noqa: F401
from loco_edit_amd.config import TINY_ADM, synth_params
from loco_edit_amd.tloco import cond_params, diffedit_rule

BAND = 1e-2        # pixels whose reference ||z| - 0.5| is below this may flip (tests/test_gpu_diffedit.py, test 4)


@pytest.fixture(scope="module")
def setup(golden):
    tiny, g = golden("tloco_tiny"), golden("tloco_diffedit")
    p = orc.to_torch(synth_params(TINY_ADM, 0))
    p.update({k: torch.from_numpy(v) for k, v in cond_params(TINY_ADM, tiny["cond_dim"], 0).items()})
    ot = tl.OracleTLoco(p, TINY_ADM, guidance_scale=g["guidance_scale"], guidance_scale_edit=g["guidance_scale_edit"])
    return tiny, g, ot


def test_fixture_describes_the_stated_inputs(golden):
    """The inputs the fixture was generated from, and the figures they give under the reference alone."""
    g = golden("tloco_diffedit")
    gx = torch.Generator().manual_seed(11)
    assert torch.equal(g["x0"], torch.randn(1, 3, 32, 32, generator=gx).clamp(-1, 1))
    assert torch.equal(g["noise"], torch.randn(10, 3, 32, 32, generator=gx))
    m, mask = g["m"], g["mask"]
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, 32, 32) == tuple(m.shape)
    assert torch.equal(do.diffedit_threshold(m), mask)                  # the recorded map reproduces the recorded mask
    assert abs(float(do.diffedit_constant(m)) - g["c"]) < 1e-6 and abs(g["c"] + 0.539) < 1e-3
    assert abs(float(mask.float().mean()) - 0.590) < 1e-3
    assert abs(float(do.diffedit_threshold(m, "intended").float().mean()) - 0.629) < 1e-3
    band = do.band_distance(m)
    assert int((band < 1e-3).sum()) == 2 and int((band < BAND).sum()) == 19
    assert float((band < BAND).float().mean()) <= 0.03                  # the cap of the GPU test, a property of the inputs


def test_restated_mask_against_the_reference(setup):
    tiny, g, ot = setup
    mask, m = do.mask_diffedit(ot, g["x0"], g["noise"], tiny["for_e"], tiny["edit_e"], tiny["null_e"])
    assert torch.allclose(m, g["m"], rtol=1e-4, atol=1e-4)
    keep = do.band_distance(g["m"]) >= BAND
    assert torch.equal(mask[keep], g["mask"][keep])
    # the null branch cancels: g (eps_for - eps_edit) is the same map
    at = ot.sched.alphas_cumprod[do.T_DIFFEDIT]
    xt = at.sqrt() * g["x0"] + (1 - at).sqrt() * g["noise"]
    with torch.no_grad():
        d = ot.cfg_noise(xt, torch.tensor(do.T_DIFFEDIT), tiny["for_e"], tiny["edit_e"], tiny["null_e"], "(for-edit)")
    m2 = d.mean(dim=0, keepdim=True).mean(dim=1)
    assert torch.allclose(m2, g["m"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("mname", ["rect", "diffedit"])
def test_restated_masked_sampler_against_the_reference(mname, setup):
    """Batch of 2 (its first frame is the B = 1 case: the reference decodes a batch of 2 frame by frame)."""
    tiny, g, ot = setup
    mk = g["rect"] if mname == "rect" else g["mask"]
    x = do.masked_forwardsteps(ot, g["dec_in"].clone(), ot.edit_t_idx, -1, tiny["for_e"], tiny["edit_e"], tiny["null_e"], mk)
    img = do.to_uint8(x)
    assert tuple(img.shape) == (2, 32, 32, 3)
    assert int((img.int() - g["masked"][f"{mname}_b2"].int()).abs().max()) <= 1
    assert int((img[:1].int() - g["masked"][f"{mname}_b1"].int()).abs().max()) <= 1
    # the same sampler stopped after `mid_steps` steps, in floating point (the final images of this stand-in are almost
    # everywhere 0 or 255 under guidance 7.5)
    end = ot.edit_t_idx + g["mid_steps"]
    xm, _, i = do.masked_forwardsteps(ot, g["dec_in"].clone(), ot.edit_t_idx, end, tiny["for_e"], tiny["edit_e"], tiny["null_e"], mk)
    assert i == end and torch.allclose(xm, g["masked_mid"][mname], rtol=1e-3, atol=1e-4)


def test_fixture_masks_give_different_states(golden):
    g = golden("tloco_diffedit")
    a, b = g["masked_mid"]["rect"], g["masked_mid"]["diffedit"]
    assert float((a - b).abs().max()) > 1e-2 and float(((a - b).abs() > 1e-3).float().mean()) > 0.25


def test_threshold_rules_on_hand_made_maps():
    # min 1, max 3: c = min / (max - min) = 0.5
    m = torch.tensor([1.0, 1.5, 2.0, 3.0])
    assert do.diffedit_z(m).tolist() == [0.5, 1.0, 1.5, 2.5]
    assert do.diffedit_threshold(m).tolist() == [False, True, True, True]        # |z| = 0.5 rounds to 0 (half to even)
    assert do.diffedit_z(m, "intended").tolist() == [0.0, 0.25, 0.5, 1.0]
    assert do.diffedit_threshold(m, "intended").tolist() == [False, False, False, True]
    # min -3, max -1: c = -1.5; z = -1.5 rounds to -2 (True), z = -0.5 and 0.5 round to 0 (False)
    m = torch.tensor([-3.0, -2.0, -1.0, -1.75])
    assert do.diffedit_z(m).tolist() == [-1.5, -0.5, 0.5, -0.25]
    assert do.diffedit_threshold(m).tolist() == [True, False, False, False]
    assert do.diffedit_threshold(m, "intended").tolist() == [False, False, True, True]
    assert do.band_distance(m).tolist() == [1.0, 0.0, 0.0, 0.25]
    with pytest.raises(ValueError):
        do.diffedit_threshold(torch.full((4,), 0.25))
    with pytest.raises(ValueError):
        do.diffedit_z(m, "other")


def test_diffedit_rule_switch(monkeypatch):
    monkeypatch.delenv("LOCO_DIFFEDIT_RULE", raising=False)
    assert diffedit_rule() == "reference"
    monkeypatch.setenv("LOCO_DIFFEDIT_RULE", "intended")
    assert diffedit_rule() == "intended"
    monkeypatch.setenv("LOCO_DIFFEDIT_RULE", "minmax")
    with pytest.raises(ValueError):
        diffedit_rule()


def test_diffedit_symbols_and_rule_codes():
    from loco_edit_amd.hip import SYMBOLS, DIFFEDIT_RULES
    assert {"loco_diffedit_mask", "loco_cfg_masked_step"} <= set(SYMBOLS)
    assert DIFFEDIT_RULES == {"reference": 0, "intended": 1}
