"""TEST INFRASTRUCTURE -- CPU restatement of the reference's DiffEdit pieces on the DeepFloyd-IF path (reference
``src/modules/edit.py`` class ``EditDeepFloydIF``): the mask derived from the two prompts (``mask_diffedit`` :1395-1407)
and the masked sampler (``MaskedDDPMforwardsteps`` :1486-1563).  Used only by tests/ and the golden generator
(oracle/make_golden_tloco_diffedit.py asserts it against the reference's own methods); the product path never imports it.
The denoiser and the guidance are those of ``tloco_oracle.OracleTLoco``.
"""
from __future__ import annotations

import torch

T_DIFFEDIT = 500        # edit.py:1396
N_DRAWS = 10            # edit.py:1398


def diffedit_map(eps_1: torch.Tensor, eps_2: torch.Tensor) -> torch.Tensor:
    """edit.py:1401: the difference of the two guided predictions [B, C, H, W], averaged over the batch, then over the
    channels -> [1, H, W]."""
    return (eps_1 - eps_2).mean(dim=0, keepdim=True).mean(dim=1)


def diffedit_constant(m: torch.Tensor) -> torch.Tensor:
    """The constant edit.py:1402 subtracts: min / (max - min) -- its parentheses divide before they subtract."""
    return m.min() / (m.max() - m.min())


def diffedit_z(m: torch.Tensor, rule: str = "reference") -> torch.Tensor:
    """The quantity that is rounded.  'reference': m - min / (max - min) (edit.py:1402 as written); 'intended':
    (m - min) / (max - min)."""
    if rule == "reference":
        return m - diffedit_constant(m)
    if rule == "intended":
        return (m - m.min()) / (m.max() - m.min())
    raise ValueError(rule)


def diffedit_threshold(m: torch.Tensor, rule: str = "reference") -> torch.Tensor:
    """edit.py:1402: round (half to even) and convert to bool -- True where the rounded value is not zero.  For the
    'intended' rule z lies in [0, 1], so that is z > 0.5; for the 'reference' rule it is |z| > 0.5."""
    if float(m.max()) == float(m.min()):
        raise ValueError("constant map: max == min (the reference divides by zero here)")
    return torch.round(diffedit_z(m, rule)).to(torch.bool)


def band_distance(m: torch.Tensor, rule: str = "reference") -> torch.Tensor:
    """How far each pixel's z is from the value at which its mask bit flips (0.5 in |z|, resp. z)."""
    z = diffedit_z(m, rule)
    return ((z.abs() if rule == "reference" else z) - 0.5).abs()


@torch.no_grad()
def mask_diffedit(ot, x0, noise, for_e, edit_e, null_e, rule: str = "reference"):
    """edit.py:1395-1407 with the ten draws injected -> (mask bool [1, H, W], map [1, H, W]).  ``ot``: an OracleTLoco."""
    t = torch.tensor(T_DIFFEDIT)
    at = ot.sched.alphas_cumprod[T_DIFFEDIT]
    xt = at.sqrt() * x0 + (1 - at).sqrt() * noise
    eps_1 = ot.cfg_noise(xt, t, for_e, edit_e, null_e, "null+(for-null)")
    eps_2 = ot.cfg_noise(xt, t, for_e, edit_e, null_e, "null+(edit-null)")
    m = diffedit_map(eps_1, eps_2)
    return diffedit_threshold(m, rule), m


@torch.no_grad()
def masked_forwardsteps(ot, xt, t_start_idx, t_end_idx, for_e, edit_e, null_e, mask):
    """edit.py:1486-1563 (eta = 0): per step the update under 'null+(for-null)' and under 'null+(edit-null)', blended by the
    mask.  Returns x_t at t_end_idx or the final sample before the uint8 conversion."""
    mk = mask.to(xt.dtype)
    do_cfg = ot.guidance_scale > 1.0
    ot.sched.set_timesteps(ot.for_steps)
    for t_idx, t in enumerate(ot.sched.timesteps):
        if t_idx < t_start_idx:
            continue
        elif t_start_idx == t_idx:
            pass
        elif t_idx == t_end_idx:
            return xt, t, t_idx
        c = xt.shape[1]
        e_for = ot.cfg_noise(xt, t, for_e, edit_e, null_e, "null+(for-null)", do_cfg=do_cfg)[:, :c]
        e_edit = ot.cfg_noise(xt, t, for_e, edit_e, null_e, "null+(edit-null)", do_cfg=do_cfg)[:, :c]
        xt = ot.sched.step(e_edit, t, xt) * mk + ot.sched.step(e_for, t, xt) * (1 - mk)
    return xt


def to_uint8(x: torch.Tensor) -> torch.Tensor:
    """edit.py:1560-1562."""
    return ((x / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)
