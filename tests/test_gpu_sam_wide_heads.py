"""GPU test of the second output channel of enc_attn_kernel (csrc/encoder_kernels.hip) with SAM's bias tables: heads wider than 64, where a lane
accumulates channel c and channel c + 64 (ViT-H has heads of 80; the kernel's LDS ends the range near 100).

Three tiny geometries with seeded weights, heads of 80, 96 and 65: grid 10, window 4 (the windows pad 10 -> 12, 16 keys: one
partial chunk of 64) and one global layer (100 keys: a full chunk and a partial one), 16 queries per workgroup so the global
layer has a partial last query block.  Reference: the torch statement of test_sam_host.py in float64 on the host; e_ref is
that statement in fp32 against it; bound max(4 e_ref, 2e-5), the bar of the tiny fixtures."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loco_edit_amd  # noqa: E402,F401
from loco_edit_amd import mask_segmentation as ms  # noqa: E402

pytestmark = pytest.mark.gpu
_spec = importlib.util.spec_from_file_location("sam_host", os.path.join(ROOT, "tests", "test_sam_host.py"))
_host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_host)


@pytest.mark.parametrize("heads,head_dim", [(2, 80), (1, 96), (2, 65)])
def test_heads_wider_than_64_vs_host_statement_float64(heads, head_dim):
    from loco_edit_amd.hip import LocoSamEngine
    cfg = ms.SamVisionConfig(image_size=40, patch_size=4, hidden_size=heads * head_dim, num_hidden_layers=3,
                             num_attention_heads=heads, mlp_dim=96, window_size=4, global_attn_indexes=(1,), output_channels=32,
                             num_pos_feats=16)
    assert cfg.head_dim == head_dim and cfg.grid == 10
    vis = _host.synthetic_vision_sd(cfg, seed=100 + head_dim)
    pv = torch.randn(3, 40, 40, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        ref = _host.restated_sam_encoder(vis, cfg, pv, torch.float64)
        e_ref = _host.rel(_host.restated_sam_encoder(vis, cfg, pv), ref)
    eng = LocoSamEngine(cfg, device=torch.device("cuda:0"))
    eng.load_state_dict(vis)
    out = eng.encode(pv)
    assert tuple(out.shape) == (1, 32, 10, 10) and torch.isfinite(out).all()
    e = _host.rel(out, ref)
    print(f"heads of {head_dim}: HIP encoder vs float64 host statement {e:.2e}   e_ref (fp32 statement) {e_ref:.2e}   "
          f"ratio {e / e_ref:.2f}")
    assert e <= _host.bound(e_ref)
    # every channel of a wide head reaches the output: zeroing v's channels >= 64 of each head moves it
    cut = {k: v.clone() for k, v in vis.items()}
    D = cfg.hidden_size
    for i in range(cfg.num_hidden_layers):
        for h in range(heads):
            rows = slice(2 * D + h * head_dim + 64, 2 * D + (h + 1) * head_dim)
            cut[f"layers.{i}.attn.qkv.weight"][rows] = 0
            cut[f"layers.{i}.attn.qkv.bias"][rows] = 0
    with torch.no_grad():
        moved = _host.rel(_host.restated_sam_encoder(cut, cfg, pv, torch.float64), ref)
    assert moved > 1e-3                                        # so an error in those channels cannot hide under the bound


def test_a_head_too_wide_for_the_lds_is_refused_at_create():
    from loco_edit_amd.hip import LocoSamEngine
    cfg = ms.SamVisionConfig(image_size=40, patch_size=4, hidden_size=128, num_hidden_layers=1, num_attention_heads=1, mlp_dim=96,
                             window_size=4, global_attn_indexes=(0,), output_channels=32, num_pos_feats=16)
    with pytest.raises(RuntimeError, match="too large for the attention kernel's LDS"):
        LocoSamEngine(cfg, device=torch.device("cuda:0"))
