"""CPU: the restatement tests/asyrp_oracle.py against torch itself, in float64 -- the hand-written backward formulas of the
Asyrp block (the ones csrc/asyrp.hip implements) against autograd, and its Adam against torch.optim.Adam over 5 steps --
and the host side of the binding (symbol list, seeded initial state)."""
import pytest
import torch

import asyrp_oracle as ao

SHAPES = [(1, 64, 8, 8, 128), (3, 96, 4, 4, 64)]


def _inputs(B, C, H, W, E, dtype=torch.float64):
    gen = torch.Generator().manual_seed(B * 1000 + C)
    h = (10 + torch.randn(B, C, H, W, generator=gen)).to(dtype)
    e = torch.randn(E, generator=gen).to(dtype)
    g = torch.randn(B, C, H, W, generator=gen).to(dtype)
    return h, e, g


@pytest.mark.parametrize("shape", SHAPES)
def test_hand_backward_matches_autograd(shape):
    B, C, H, W, E = shape
    p = ao.random_params(C, E, seed=3, dtype=torch.float64)
    h, e, g = _inputs(*shape)
    _, gh_ref, grads_ref = ao.block_grads(p, h, e, g, s=0.7)
    gh, grads = ao.block_backward(p, h, e, g, s=0.7)
    assert ao.rel_err(gh, gh_ref) < 1e-12
    for k in ao.PARAMS:
        assert ao.rel_err(grads[k], grads_ref[k]) < 1e-12, k


def test_zero_tail_is_identity_edit():
    B, C, H, W, E = SHAPES[0]
    p = ao.random_params(C, E, seed=1, dtype=torch.float64)
    p["W2"].zero_()
    p["c2"].zero_()
    h, e, _ = _inputs(*SHAPES[0])
    assert not ao.block_forward(p, h, e).any()


def test_adam_matches_torch():
    gen = torch.Generator().manual_seed(0)
    p0 = {"a": torch.randn(7, 5, generator=gen, dtype=torch.float64), "b": torch.randn(11, generator=gen, dtype=torch.float64)}
    ref = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    topt = torch.optim.Adam(list(ref.values()), lr=3e-2, betas=(0.9, 0.999), eps=1e-8)
    opt = ao.Adam(p0, lr=3e-2)
    for step in range(5):
        grads = {k: torch.randn(v.shape, generator=gen, dtype=torch.float64) * (step + 1) for k, v in p0.items()}
        for k in ref:
            ref[k].grad = grads[k].clone()
        topt.step()
        opt.step(grads)
        for k in ref:
            assert ao.rel_err(opt.p[k], ref[k].detach()) < 1e-13, (step, k)


def test_binding_lists_the_unit():
    from loco_edit_amd import hip
    names = {"create", "destroy", "last_error", "load_param", "read_param", "forward", "backward", "zero_grad", "read_grad", "adam_step"}
    assert {f"loco_asyrp_{n}" for n in names} <= set(hip.SYMBOLS)
    assert hip.LocoAsyrpBlock.PARAMS == ao.PARAMS
    assert hip.LocoAsyrpBlock.param_shapes(64, 128) == ao.param_shapes(64, 128)


def test_initial_state_is_seeded_and_an_identity_edit():
    from loco_edit_amd.hip import LocoAsyrpBlock
    a, b, c = LocoAsyrpBlock.init_params(64, 128, seed=4), LocoAsyrpBlock.init_params(64, 128, seed=4), LocoAsyrpBlock.init_params(64, 128, seed=5)
    assert all(torch.equal(a[k], b[k]) for k in ao.PARAMS)
    assert not torch.equal(a["W1"], c["W1"])
    assert not a["W2"].any() and not a["c2"].any()
    assert {k: tuple(v.shape) for k, v in a.items()} == ao.param_shapes(64, 128)
    h, e, _ = _inputs(1, 64, 8, 8, 128, torch.float32)
    assert not ao.block_forward(a, h, e).any()


# ------------------------------------------------------------------------------------------- loco_edit_amd/asyrp.py, host side
BASE = ["--sh_file_name", "x.sh", "--model_name", "CelebA_HQ_HF", "--dataset_name", "Synthetic"]


def test_directional_cosine_gradient_matches_autograd():
    from loco_edit_amd import asyrp
    gen = torch.Generator().manual_seed(2)
    emb = torch.randn(2, 24, generator=gen, dtype=torch.float64)
    ts, tt = torch.randn(24, generator=gen, dtype=torch.float64), torch.randn(24, generator=gen, dtype=torch.float64)
    e = emb.clone().requires_grad_(True)
    want = ao.directional_loss(e[0], e[1].detach(), ts, tt)
    want.backward()
    loss, g = asyrp.directional_cosine(emb, tt - ts)
    assert abs(float(loss) - float(want.detach())) < 1e-14
    assert ao.rel_err(g[0], e.grad[0]) < 1e-12 and not g[1].any()
    assert asyrp.DIR_EPS == ao.DIR_EPS
    # an untrained block: both frames embed alike, the loss is 1 and the gradient finite, along the text direction
    loss0, g0 = asyrp.directional_cosine(torch.stack([emb[1], emb[1]]), tt - ts)
    tn = (tt - ts) / (tt - ts).norm()
    assert float(loss0) == 1.0 and torch.allclose(g0[0], -tn / asyrp.DIR_EPS, rtol=1e-12) and not g0[1].any()


def test_time_vector_follows_the_denoisers_convention():
    from loco_edit_amd import asyrp
    from loco_edit_amd.config import TINY_ADM, TINY_DDPM, TINY_DECODER
    for cfg in (TINY_DDPM, TINY_ADM):
        for t in (1.0, 601.0, 999.0):
            e = asyrp.time_vector(cfg, t)
            assert e.dtype == torch.float32 and tuple(e.shape) == (cfg.temb_ch,)
            assert torch.equal(e, ao.time_vector(cfg, t, torch.float32))
    assert not torch.equal(asyrp.time_vector(TINY_DDPM, 601.0)[:4], asyrp.time_vector(TINY_ADM, 601.0)[:4])
    with pytest.raises(ValueError, match="h-space tap"):
        asyrp.time_vector(TINY_DECODER, 1.0)


def test_asymmetric_step_restatement_reduces_to_ddim():
    gen = torch.Generator().manual_seed(4)
    x, e1, e2 = (torch.randn(1, 3, 8, 8, generator=gen, dtype=torch.float64) for _ in range(3))
    at, an = 0.37, 0.52
    same = ao.asym_step(x, e1, e1, at, an)
    ddim = an ** 0.5 * ((x - (1 - at) ** 0.5 * e1) / at ** 0.5) + (1 - an) ** 0.5 * e1
    assert torch.equal(same, ddim)
    mixed = ao.asym_step(x, e1, e2, at, an)
    assert torch.allclose(mixed - same, (1 - an) ** 0.5 * (e2 - e1), atol=1e-14)


def test_index_ranges():
    from loco_edit_amd.asyrp import parse_index_range
    assert parse_index_range("0-3") == [0, 1, 2, 3] and parse_index_range("5") == [5] and parse_index_range("3,7-8") == [3, 7, 8]
    for bad in ("", "a-b", "4-2", "-1"):
        with pytest.raises(ValueError, match="asyrp_train_idx"):
            parse_index_range(bad)


def test_flag_defaults_and_refusals():
    from loco_edit_amd.define_argparser import parse_args
    args = parse_args(BASE)
    assert not args.run_edit_asyrp
    assert (args.asyrp_epochs, args.asyrp_lr, args.asyrp_clip_weight, args.asyrp_rec_weight, args.asyrp_scale) == (1, 1e-3, 0.8, 3.0, 1.0)
    on = BASE + ["--run_edit_asyrp", "True"]
    pair = ["--asyrp_src_prompt", "a face", "--asyrp_tgt_prompt", "a smiling face"]
    with pytest.raises(ValueError, match="--run_edit_asyrp needs --clip_model_path"):
        parse_args(on + pair)
    with pytest.raises(ValueError, match="--asyrp_src_prompt and --asyrp_tgt_prompt"):
        parse_args(on + ["--clip_model_path", "/nowhere", "--asyrp_tgt_prompt", "a smiling face"])
    with pytest.raises(ValueError, match="no direction"):
        parse_args(on + ["--clip_model_path", "/nowhere", "--asyrp_src_prompt", "a", "--asyrp_tgt_prompt", "a"])
    with pytest.raises(ValueError, match="asyrp_lr"):
        parse_args(on + pair + ["--clip_model_path", "/nowhere", "--asyrp_lr", "0"])
    with pytest.raises(ValueError, match="asyrp_train_idx"):
        parse_args(on + pair + ["--clip_model_path", "/nowhere", "--asyrp_train_idx", "9-2"])
    with pytest.raises(ValueError, match="unconditional"):
        parse_args(["--sh_file_name", "x.sh", "--model_name", "stable-diffusion-v1-5", "--dataset_name", "Random", "--run_edit_asyrp", "True",
                    "--clip_model_path", "/nowhere"] + pair)
    ok = parse_args(on + pair + ["--clip_model_path", "/nowhere", "--asyrp_train_idx", "0-1", "--asyrp_scale", "1.5"])
    assert ok.run_edit_asyrp and ok.asyrp_scale == 1.5


def test_loss_refuses_a_scorer_without_records():
    from types import SimpleNamespace
    from loco_edit_amd import asyrp
    x = torch.zeros(1, 3, 8, 8)
    plain = SimpleNamespace(vision=SimpleNamespace(grad=False, max_images=2))
    with pytest.raises(RuntimeError, match="grad=True"):
        asyrp.directional_clip_loss(plain, x, x, torch.zeros(4), torch.zeros(4))
    one = SimpleNamespace(vision=SimpleNamespace(grad=True, max_images=1))
    with pytest.raises(RuntimeError, match="max_images >= 2"):
        asyrp.directional_clip_loss(one, x, x, torch.zeros(4), torch.zeros(4))
    two = SimpleNamespace(vision=SimpleNamespace(grad=True, max_images=2), vision_cfg=SimpleNamespace(projection_dim=4))
    with pytest.raises(ValueError, match=r"\[1, 3, H, W\]"):
        asyrp.directional_clip_loss(two, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), torch.zeros(4), torch.zeros(4))
    with pytest.raises(ValueError, match="text embeddings must hold 4"):
        asyrp.directional_clip_loss(two, x, x, torch.zeros(5), torch.zeros(4))
