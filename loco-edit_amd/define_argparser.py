"""Flags and derived settings of the unconditional LOCO-Edit path: the subset of
reference ``src/utils/define_argparser.py:14-258``: the complete flag schema (same
names / types / defaults, so every shipped ``scripts/main_*.sh`` argument list
parses), the derived fields of ``preset`` for the unconditional branch, plus the
deployment flags ``--ckpt_path``, ``--synthetic_weights``, ``--max_batch``, ``--precision``.
"""
import argparse
import os
import random
import shutil

import numpy as np
import torch


def str2bool(v):
    """define_argparser.py:128-136."""
    if isinstance(v, bool):
        return v
    if v.lower() in ('true'):
        return True
    elif v.lower() in ('false'):
        return False
    else:
        raise argparse.ArgumentTypeError('Boolean value expected.')


# Flag schema = reference define_argparser.py:18-124 (every flag the twelve shipped scripts pass parses here with
# the reference's name, type and default); rows: (name, type, default).  Flags that only steer subsystems outside
# the unconditional hot path (prompts, guidance scales, SAM model name, ablations) are accepted and carried on the
# Namespace so the shipped scripts run unmodified; `preset` rejects the text-to-image model names.
_S, _I, _F = str, int, float
_FLAGS = [
    # default setting
    ('sh_file_name', _S, ''), ('device', _S, 'cuda:0'), ('dtype', _S, 'fp32'), ('seed', _I, 0),
    ('result_folder', _S, './runs/'), ('cache_folder', _S, ''), ('dataset_root', _S, ''),
    # model, dataset
    ('model_name', _S, 'CelebA_HQ_HF'), ('dataset_name', _S, 'Synthetic'), ('num_imgs', _I, 100),
    ('image_size', _I, 256), ('c_in', _I, 3), ('sample_idx', _I, 0),
    # prompts (text-to-image only)
    ('for_prompt', _S, ''), ('inv_prompt', _S, ''), ('neg_prompt', _S, ''),
    # diffusion schedule
    ('for_steps', _I, 100), ('inv_steps', _I, 100), ('performance_boosting_t', _F, 0.0),
    ('use_yh_custom_scheduler', 'bool', 'True'),
    # guidance (text-to-image only)
    ('guidance_scale', _F, 0), ('guidance_scale_edit', _F, 4.0),
    # edit
    ('edit_prompt', _S, ''), ('original_prompt', _S, ''), ('edit_xt', _S, 'default'),
    ('use_x_space_guidance', 'bool', 'False'), ('x_space_guidance_direct', 'bool', 'False'),
    ('x_space_guidance_edit_step', _F, 1), ('x_space_guidance_scale', _F, 0), ('x_space_guidance_num_step', _I, 0),
    ('x_space_guidance_use_edit_prompt', 'bool', 'True'), ('pca_rank_null', _I, 5), ('pca_rank', _I, 5),
    ('h_t', _F, 0.8), ('edit_t', _F, 1.0), ('no_edit_t', _F, 0.5), ('h_edit_step_size', _F, 0),
    ('x_edit_step_size', _F, 0),
    # memory (accepted for script compatibility; batches stay in HBM)
    ('pca_device', _S, 'cpu'), ('buffer_device', _S, 'cpu'), ('save_result_as', _S, 'image'),
    # experiments
    ('note', _S, None),
    ('run_cfg_forward', 'bool', 'False'), ('run_mcg_forward', 'bool', 'False'), ('run_pfg_forward', 'bool', 'False'),
    ('run_ddim_forward', 'bool', 'False'), ('run_ddim_inversion', 'bool', 'False'),
    ('run_edit_local_encoder_pullback_zt', 'bool', 'False'), ('run_edit_local_decoder_pullback_zt', 'bool', 'False'),
    ('run_edit_local_encoder_decoder_pullback_zt', 'bool', 'False'), ('encoder_decoder_by_et', 'bool', 'False'),
    ('use_mask', 'bool', 'True'), ('run_edit_local_x0_decoder_pullback_zt', 'bool', 'False'),
    ('run_edit_local_pca_zt', 'bool', 'False'), ('run_edit_null_space_projection', 'bool', 'False'),
    ('run_edit_null_space_projection_zt', 'bool', 'False'),
    ('run_edit_null_space_projection_zt_semantic', 'bool', 'False'),
    ('run_edit_null_space_projection_xt', 'bool', 'False'),
    ('run_edit_null_space_projection_xt_semantic', 'bool', 'False'),
    ('group_edit_null_space_projection', 'bool', 'False'), ('run_edit_blended_diffusion', 'bool', 'False'),
    ('vis_num', _I, 4), ('choose_sem', _S, 'hair'), ('null_space_projection', 'bool', 'False'),
    # mode
    ('debug_mode', 'bool', 'False'), ('sampling_mode', 'bool', 'False'), ('non_semantic', 'bool', 'False'),
    # mask segmentation
    ('mask_model_name', _S, 'facebook/sam-vit-large'), ('filter_mask', _I, 100), ('mask_index', _I, 0),
    ('vT_path', _S, ''), ('vT1_path', _S, ''), ('jacobian', 'bool', 'False'), ('use_sega', 'bool', 'False'),
    ('edit_t_idx', _I, 1), ('num_inference_steps', _I, 3), ('random_edit', 'bool', 'False'),
]
_UNET_PRESETS = {'celeba_ddpm': 'CELEBA_DDPM', 'ffhq_p2': 'FFHQ_P2', 'tiny_ddpm': 'TINY_DDPM', 'mid_ddpm': 'MID_DDPM',
                 'tiny_adm': 'TINY_ADM', 'if64_standin': 'IF64_STANDIN', 'sd64_standin': 'SD64_STANDIN',
                 'sd64_xattn_standin': 'SD64_XATTN_STANDIN', 'tiny_latent': 'TINY_LATENT', 'tiny_latent_xattn': 'TINY_LATENT_XATTN',
                 'if64_xattn_standin': 'IF64_XATTN_STANDIN', 'tiny_adm_xattn': 'TINY_ADM_XATTN', 'sd15_unet': 'SD15_UNET', 'sd21_base_unet': 'SD21_BASE_UNET',
                 'tiny_ldm': 'TINY_LDM', 'if_i_m_unet': 'IF_I_M_UNET', 'tiny_if': 'TINY_IF', 'mid_if': 'MID_IF',
                 'lcm_dreamshaper_v7_unet': 'LCM_DREAMSHAPER_V7_UNET', 'tiny_lcm': 'TINY_LCM'}
_VAE_PRESETS = {'sd_vae_decoder': 'SD_VAE_DECODER', 'tiny_decoder': 'TINY_DECODER'}
_TILDA_V = ["proj_null[for-null](edit-null)-direct", "(for-edit)-direct", "(edit-null)-direct",
            "null+(for-null)+(edit-null)", "null+(for-null)", "null+(edit-null)", "(for-edit)",
            "edit-proj[for](edit)", "null+for+edit-proj[for](edit)"]


def build_parser():
    p = argparse.ArgumentParser()
    for name, typ, default in _FLAGS:
        p.add_argument('--' + name, type=str2bool if typ == 'bool' else typ, default=default)
    p.add_argument('--mask_type', type=str, default="SAM", choices=["SAM", "diffedit"])
    p.add_argument('--ablation_method', type=str, choices=["null-space-proj", "sega", "diffedit"])
    p.add_argument('--tilda_v_score_type', type=str, choices=_TILDA_V)
    # deployment flags of this build (not in the reference)
    p.add_argument('--ckpt_path', type=str, default='', help='state_dict in the vendored Ho-DDPM / ADM / diffusers key layout')
    p.add_argument('--synthetic_weights', type=int, default=None, help='seed of the deterministic weight synthesiser')
    p.add_argument('--max_batch', type=int, default=0,
                   help='largest image/probe batch resident on the GPU per pass; 0 = from the probe counts: '
                        'clamp(pca_rank + pca_rank_null, 8, 32) for the unconditional models (about 1 GB of arena per '
                        'probe at 256x256; wider batches fill the deep levels: 64 probes run 9 %% faster at 32 than at 8), '
                        '8 for the text-to-image paths (several engine contexts)')
    p.add_argument('--unet_preset', type=str, default=None, choices=sorted(_UNET_PRESETS),
                   help='override the architecture --model_name implies (small parity-test sizes)')
    p.add_argument('--vae_preset', type=str, default=None, choices=sorted(_VAE_PRESETS),
                   help='latent T-LOCO: decoder architecture (default: the Stable Diffusion autoencoder decoder geometry)')
    p.add_argument('--vae_ckpt_path', type=str, default='', help='latent T-LOCO: decoder state_dict in latent-diffusion `Decoder` naming')
    p.add_argument('--prompt_emb_path', type=str, default='',
                   help="T-LOCO: torch file {'for','edit','null': [1, tokens, D]} of prompt embeddings (or --text_encoder_path)")
    p.add_argument('--text_encoder_path', type=str, default='',
                   help='text encoder that turns --for_prompt / --edit_prompt / ... into prompt states on the GPU -- Stable '
                        'Diffusion: CLIP; DeepFloyd IF: T5 (v1.1 encoder, fp32; prompts lower-cased and stripped, 77 tokens). A '
                        'diffusers pipeline root (text_encoder/ + tokenizer/), a text_encoder/ folder (one file or a sharded '
                        '*.index.json checkpoint) or a single state_dict file (CompVis SD 1.x .ckpt); the kind is read from the '
                        'checkpoint and must fit the model; excludes --prompt_emb_path')
    p.add_argument('--tokenizer_path', type=str, default='',
                   help='tokenizer folder when --text_encoder_path is not a pipeline root: CLIP (vocab.json, merges.txt, configs) '
                        'or T5 (tokenizer.json with a Unigram model, or spiece.model)')
    p.add_argument('--mask_model_path', type=str, default='',
                   help='Segment Anything model that produces mask/mask.pt on the GPU when it is missing: a local SamModel '
                        'folder (config.json + model.safetensors or pytorch_model.bin) or a checkpoint file in SamModel naming. '
                        'Nothing is downloaded (--mask_model_name stays a name only). Empty: mask/mask.pt must exist')
    p.add_argument('--mask_head', type=str, default='torch', choices=['torch', 'hip'],
                   help='prompt encoder / mask decoder / mask filters behind --mask_model_path: torch (functions on the device) or '
                        'hip (the kernels of csrc/samdec.hip)')
    p.add_argument('--clip_model_path', type=str, default='',
                   help='T-LOCO semantic edits: CLIP model that scores the returned frames on the GPU (image-text cosine with '
                        '--for_prompt / --edit_prompt, cosine with the unedited frame, directional similarity) into '
                        '<result_folder>/<EXP_NAME>_clip.json: a local transformers CLIPModel folder (config.json + '
                        'model.safetensors or pytorch_model.bin, its tokenizer files or --tokenizer_path) or a state_dict file. '
                        'Empty: no scores, nothing else changes')
    p.add_argument('--clip_preprocess', type=str, default='device', choices=['pil', 'device'],
                   help="--clip_model_path: 'device' resizes the frames on the GPU in float arithmetic, 'pil' on the host with PIL "
                        "(CLIPImageProcessor's input exactly)")
    p.add_argument('--quality_metrics', type=str, default='',
                   help='score the decoded frames of an edit on the GPU against the unedited frame into '
                        '<result_folder>/<name>_quality.json: a comma list drawn from ssim,mmse,lpips (mmse: MSE inside the '
                        "run's mask and outside it). Empty: no scores, nothing else changes")
    p.add_argument('--lpips_weights', type=str, default='',
                   help="--quality_metrics lpips: a state dict with torchvision AlexNet's features.* and the lpips package's "
                        "lin*.model.1.weight heads, or 'features_file,heads_file'; no pretrained weights are available offline "
                        'and without them lpips raises')
    p.add_argument('--lcm_timesteps', type=str, default=None, choices=['linspace', 'stride'],
                   help='latent-consistency models (required for them): which published LCMScheduler.set_timesteps rule picks the '
                        "N sampling timesteps out of the 50 training ones -- 'linspace' (current diffusers: N = 4 gives "
                        "[999, 759, 499, 259]) or 'stride' (LCMScheduler as first released: [999, 759, 519, 279]); the reference "
                        'does not pin a diffusers version that has the scheduler')
    p.add_argument('--cond_dim', type=int, default=16, help='T-LOCO stand-in: width of seeded prompt embeddings when no file is given')
    p.add_argument('--precision', type=str, default=None, choices=['f32', 'bf16x3', 'f16'],
                   help="conv arithmetic of the HIP engine: 'f32' exact fp32 MFMA (parity anchor), 'bf16x3' split-bf16 "
                        "(fp32-faithful to ~2^-16, default), 'f16' single f16 MFMA with fp32 accumulate (2^-11 operands; opt-in: "
                        "operands are cast without range management, so tangent / cotangent entries below 6e-5 lose bits and "
                        "above 65504 overflow -- pinned on synthetic weights only)")
    p.add_argument('--solver', type=str, default=None, choices=['power', 'krylov'],
                   help="basis solver (sets LOCO_SOLVER): 'power' block power iteration (default, the reference's loop), 'krylov' "
                        "block Krylov with Rayleigh-Ritz over all iterates: same two passes per step, stops on its own test, at most "
                        "32 probes per solve; writes <basis name>_residual.json next to each basis it computes")
    p.add_argument('--jacobian_target', type=str, default='x0', choices=['x0', 'h'],
                   help="--run_edit_null_space_projection: what the modify-space basis is the pullback of. 'x0' (default): the "
                        "masked posterior mean, LOCO. 'h': the U-Net bottleneck (the Pullback baseline, d h / d x_t, no mask in that "
                        "solve); the null-space solve, projection, edit walk and --vT_path are the same, basis and result names "
                        "gain an -hspace tag. Unconditional models, --run_edit_null_space_projection and the power "
                        "solver only: refused with another driver or with --solver krylov")
    p.add_argument('--clip_guidance_scale', type=float, default=1000.0,
                   help='--run_edit_blended_diffusion: weight of the CLIP loss mean_i (1 - cos) (the released Blended Diffusion default)')
    p.add_argument('--blended_num_aug', type=int, default=8,
                   help='--run_edit_blended_diffusion: windows of the masked x0 estimate the CLIP loss averages over per step (the '
                        'first is the whole frame, the others squares of 0.75 - 1 of the short side)')
    p.add_argument('--blended_start_t', type=float, default=0.5,
                   help='--run_edit_blended_diffusion: the noise level (fraction of the 1000 training steps) the source image is '
                        'taken to; the run starts at the nearest timestep of the --for_steps schedule')
    p.add_argument('--range_scale', type=float, default=50.0,
                   help='--run_edit_blended_diffusion: weight of the range loss mean |x0 - clamp(x0, -1, 1)|')
    p.add_argument('--run_edit_hspace_pca', type=str2bool, default=False,
                   help='edit along unsupervised h-space directions: PCA of the U-Net bottleneck h at --edit_t, computed on the '
                        'device (the global / local h-space PCA baselines). Unconditional models only; --pca_rank directions are '
                        'shown, --vis_num frames each side')
    p.add_argument('--hspace_pca', type=str, default='global', choices=['global', 'local'],
                   help="--run_edit_hspace_pca: 'global' = PCA of h over --hspace_pca_samples fresh x_T taken to --edit_t; 'local' = "
                        "PCA of h over that many unit-norm perturbations of the inverted image's x_t")
    p.add_argument('--hspace_pca_samples', type=int, default=1000,
                   help='--run_edit_hspace_pca: samples of h the PCA is taken over (the reference default is 50000)')
    p.add_argument('--hspace_pca_rank', type=int, default=50,
                   help='--run_edit_hspace_pca: rank of the PCA, at most min(samples - 1, 512); --pca_rank of them are shown')
    p.add_argument('--hspace_edit', type=str, default='h', choices=['h', 'x'],
                   help="--run_edit_hspace_pca: 'h' adds alpha * scale * s_k / sqrt(N - 1) * u_k to h at every remaining step of the "
                        "decode; 'x' moves x_t along inv_jac_xt(u_k) as --run_edit_null_space_projection moves it along its basis")
    p.add_argument('--hspace_edit_scale', type=float, default=1.0,
                   help='--run_edit_hspace_pca --hspace_edit h: multiplies the walk, in standard deviations of h along the direction')
    p.add_argument('--run_edit_asyrp', type=str2bool, default=False,
                   help='the Asyrp baseline: train a small h-space block f_t from one text pair (--asyrp_src_prompt, '
                        '--asyrp_tgt_prompt) with a directional CLIP loss on the device, then edit --sample_idx with the asymmetric '
                        'DDIM step from T down to --edit_t. Unconditional models only; needs --clip_model_path')
    p.add_argument('--asyrp_src_prompt', type=str, default='', help='--run_edit_asyrp: the text of the source attribute, e.g. "a face"')
    p.add_argument('--asyrp_tgt_prompt', type=str, default='', help='--run_edit_asyrp: the text of the target attribute, e.g. "a smiling face"')
    p.add_argument('--asyrp_ckpt', type=str, default='',
                   help='--run_edit_asyrp: the trained block (a state dict of its ten tensors plus the Adam step count): loaded when '
                        'the file exists, else trained and saved there. Empty: <result_folder>/asyrp_ckpt.pt')
    p.add_argument('--asyrp_train_idx', type=str, default='0-99',
                   help='--run_edit_asyrp: the dataset images the block is trained on, e.g. 0-99 or 3,7,11 (inclusive ranges)')
    p.add_argument('--asyrp_epochs', type=int, default=1, help='--run_edit_asyrp: passes over the training images')
    p.add_argument('--asyrp_lr', type=float, default=1e-3,
                   help="--run_edit_asyrp: Adam's step size, constant (no scheduler is built). Asyrp publishes 0.5 with its own "
                        'scheduler; here the first Adam step moves every weight of the C x C output conv by lr with coherent signs, '
                        'which shifts h by about 0.35 C lr: 1e-3 keeps that below a fifth of the spread of h at C = 512')
    p.add_argument('--asyrp_clip_weight', type=float, default=0.8, help='--run_edit_asyrp: weight of the directional CLIP loss (as published)')
    p.add_argument('--asyrp_rec_weight', type=float, default=3.0,
                   help='--run_edit_asyrp: weight of the reconstruction loss mean |x0_edit - x0_src| (as published)')
    p.add_argument('--asyrp_scale', type=float, default=1.0, help='--run_edit_asyrp: multiplies the learned dh at inference')
    p.add_argument('--null_text_inversion', type=str2bool, default=False,
                   help='Stable Diffusion edit runs on an image of the dataset (--dataset_name other than Random, --sample_idx): DDIM '
                        'inversion under the for prompt, then null-text inversion (Mokady et al. 2023) -- the unconditional prompt '
                        'states are optimised per timestep so that the guided decode returns to the image; cached as '
                        'null_text-<idx>.pt in the result folder. Needs --inv_steps == --for_steps')
    p.add_argument('--null_text_inner_steps', type=int, default=10, help='--null_text_inversion: Adam steps per timestep at most (as published)')
    p.add_argument('--null_text_lr', type=float, default=1e-2, help='--null_text_inversion: lr of step i is this times (1 - i / 100) (as published)')
    p.add_argument('--null_text_early_stop', type=float, default=1e-5,
                   help='--null_text_inversion: the inner loop of step i stops at loss < this + 2e-5 i (as published)')
    p.add_argument('--mask_prompts', type=str, default='',
                   help='text-prompted edit masks: a comma list such as "hair,eyes,mouth"; when mask/mask.pt is missing, CLIPSeg '
                        '(--mask_prompt_model_path) writes one mask per entry, in order, so --mask_index selects a prompt')
    p.add_argument('--mask_prompt_model_path', type=str, default='',
                   help='CLIPSeg model behind --mask_prompts: a local CLIPSegForImageSegmentation folder (config.json + '
                        'model.safetensors or pytorch_model.bin, tokenizer files or --tokenizer_path, optional '
                        'preprocessor_config.json) or a state_dict file. Nothing is downloaded. Excludes --mask_model_path')
    p.add_argument('--mask_prompt_threshold', type=float, default=0.5,
                   help='--mask_prompts: a pixel belongs to the mask when sigmoid(logit) exceeds this (a user knob: lower it for a '
                        'wider mask; a prompt whose mask comes out empty is an error)')
    return p


def check_mask_prompt_args(args):
    """The combinations of --mask_prompts / --mask_prompt_model_path / --mask_model_path / --mask_index that make no sense."""
    prompts, model = getattr(args, "mask_prompts", ""), getattr(args, "mask_prompt_model_path", "")
    if model and getattr(args, "mask_model_path", ""):
        raise ValueError("--mask_model_path (Segment Anything) and --mask_prompt_model_path (CLIPSeg) both write mask/mask.pt: pass one")
    if prompts and not model:
        raise ValueError("--mask_prompts needs --mask_prompt_model_path (a local CLIPSegForImageSegmentation folder or state_dict file)")
    if model and not prompts:
        raise ValueError("--mask_prompt_model_path needs --mask_prompts (a comma list, one mask per entry)")
    if not model:
        return
    from .prompt_mask import parse_prompts, threshold_logit
    names = parse_prompts(prompts)
    threshold_logit(args.mask_prompt_threshold)
    if not 0 <= int(args.mask_index) < len(names):
        raise ValueError(f"--mask_index {args.mask_index} is beyond the {len(names)} prompts of --mask_prompts {names}")


def check_blended_args(args, edit_prompt=None):
    """--run_edit_blended_diffusion needs a CLIP model and an edit prompt: checked before any device work."""
    if not getattr(args, "clip_model_path", ""):
        raise ValueError("--run_edit_blended_diffusion needs --clip_model_path (the CLIP model whose score guides the edit)")
    if not (args.edit_prompt if edit_prompt is None else edit_prompt):
        raise ValueError("--run_edit_blended_diffusion needs --edit_prompt (the text the masked region is driven towards)")
    if not 0.0 < float(args.blended_start_t) <= 1.0:
        raise ValueError(f"--blended_start_t {args.blended_start_t}: a noise level in (0, 1]")
    if int(args.blended_num_aug) < 1:
        raise ValueError("--blended_num_aug must be at least 1")


def check_asyrp_args(args):
    """--run_edit_asyrp needs a CLIP model and the text pair: checked before any device work."""
    if any(s in args.model_name for s in ('stable-diffusion', 'DeepFloyd', 'LCM')):
        raise ValueError("--run_edit_asyrp trains on an unconditional denoiser's bottleneck: the text-to-image classes are not wired to it")
    if not getattr(args, "clip_model_path", ""):
        raise ValueError("--run_edit_asyrp needs --clip_model_path (the CLIP model whose directional loss trains the block)")
    if not args.asyrp_src_prompt or not args.asyrp_tgt_prompt:
        raise ValueError("--run_edit_asyrp needs --asyrp_src_prompt and --asyrp_tgt_prompt (the text pair the edit direction is read from)")
    if args.asyrp_src_prompt == args.asyrp_tgt_prompt:
        raise ValueError("--asyrp_src_prompt and --asyrp_tgt_prompt are the same text: the pair has no direction")
    if int(args.asyrp_epochs) < 1:
        raise ValueError("--asyrp_epochs must be at least 1")
    if not float(args.asyrp_lr) > 0 or not np.isfinite(args.asyrp_lr):
        raise ValueError(f"--asyrp_lr {args.asyrp_lr} must be positive and finite")
    if not np.isfinite(args.asyrp_scale):
        raise ValueError(f"--asyrp_scale {args.asyrp_scale} must be finite")
    from .asyrp import parse_index_range
    parse_index_range(args.asyrp_train_idx)


HSPACE_PCA_Q_LIMIT = 512          # hip.LocoPca.Q_LIMIT (not imported here: parsing needs no device library)


def check_hspace_pca_args(args):
    """--run_edit_hspace_pca and its flags: checked before any device work."""
    given = [f for f, d in (('hspace_pca', 'global'), ('hspace_pca_samples', 1000), ('hspace_pca_rank', 50), ('hspace_edit', 'h'),
                            ('hspace_edit_scale', 1.0)) if getattr(args, f) != d]
    if not args.run_edit_hspace_pca:
        if given:
            raise ValueError(f"--{given[0]} is read by --run_edit_hspace_pca only")
        return
    if any(s in args.model_name for s in ('stable-diffusion', 'DeepFloyd', 'LCM')):
        raise ValueError("--run_edit_hspace_pca is built for the unconditional models (the T-LOCO classes have no h-space tap "
                         "on their classifier-free-guidance combination)")
    if args.hspace_pca_samples < 3:
        raise ValueError(f"--hspace_pca_samples {args.hspace_pca_samples}: a centred PCA needs at least 3 samples")
    most = min(args.hspace_pca_samples - 1, HSPACE_PCA_Q_LIMIT)
    if not 1 <= args.hspace_pca_rank <= most:
        raise ValueError(f"--hspace_pca_rank {args.hspace_pca_rank} must lie in [1, min(samples - 1, {HSPACE_PCA_Q_LIMIT})] = [1, {most}]")
    if args.pca_rank > args.hspace_pca_rank:
        raise ValueError(f"--pca_rank {args.pca_rank} directions are shown, the PCA has only --hspace_pca_rank {args.hspace_pca_rank}")
    if not args.hspace_edit_scale > 0 or not np.isfinite(args.hspace_edit_scale):
        raise ValueError(f"--hspace_edit_scale {args.hspace_edit_scale} must be positive and finite")
    if args.hspace_edit == 'x' and args.hspace_edit_scale != 1.0:
        raise ValueError("--hspace_edit_scale scales the h-space walk (--hspace_edit h); the x-space walk is scaled by "
                         "--x_space_guidance_scale")
    if args.vT_path:
        raise ValueError("--vT_path loads an x-space basis for --run_edit_null_space_projection; --run_edit_hspace_pca keeps its "
                         "own basis file")


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.solver:
        os.environ["LOCO_SOLVER"] = args.solver
    check_hspace_pca_args(args)
    if args.jacobian_target == 'h':
        if any(s in args.model_name for s in ('stable-diffusion', 'DeepFloyd', 'LCM')):
            raise ValueError("--jacobian_target h is built for the unconditional models (the T-LOCO classes differentiate a "
                             "classifier-free-guidance combination)")
        if not args.run_edit_null_space_projection:
            raise ValueError("--jacobian_target h is read by --run_edit_null_space_projection only: no other driver solves for a basis")
        if os.environ.get("LOCO_SOLVER", "power") == "krylov":
            raise ValueError("--jacobian_target h runs the power iteration: the block Krylov solver (--solver krylov / LOCO_SOLVER) "
                             "is not wired to the h-space operators")
    if args.run_edit_blended_diffusion:
        if any(s in args.model_name for s in ('stable-diffusion', 'DeepFloyd', 'LCM')):
            raise ValueError("--run_edit_blended_diffusion edits with an unconditional DDPM: the text-to-image classes are not wired to it")
        check_blended_args(args)
    if args.run_edit_asyrp:
        check_asyrp_args(args)
    check_mask_prompt_args(args)
    if args.text_encoder_path and args.prompt_emb_path:
        raise ValueError("--text_encoder_path and --prompt_emb_path both give the prompt embeddings: pass one of them")
    if args.max_batch <= 0:
        t2i = any(s in args.model_name for s in ('stable-diffusion', 'DeepFloyd', 'LCM'))
        # sized by what actually shares a pass: the probes of the modify-space and null-space solves when they run as a
        # pair (solver.local_basis_pair; not with LOCO_PAIR_SOLVES=0, without projection or with a loaded basis), and the
        # edited frames of all shown directions in the decode (vis_num_pc x (2 vis_num + 1) frames at most)
        pair = (args.null_space_projection and not args.vT_path and os.environ.get("LOCO_PAIR_SOLVES", "1") != "0"
                and args.jacobian_target == 'x0')
        probes = args.pca_rank + (args.pca_rank_null if pair else 0)
        frames = args.pca_rank * (2 * max(int(args.vis_num), 1) + 1)     # main.py passes vis_num_pc = pca_rank
        args.max_batch = 8 if t2i else min(32, max(8, probes, frames))
    if args.unet_preset:
        from . import config
        args.unet_config = getattr(config, _UNET_PRESETS[args.unet_preset])
    if args.vae_preset:
        from . import config
        args.vae_config = getattr(config, _VAE_PRESETS[args.vae_preset])
    return args


UNCOND_MODELS_HF = ('CelebA_HQ_HF', 'LSUN_church_HF', 'LSUN_bedroom_HF', 'FFHQ_HF')
UNCOND_MODELS_P2 = ('FFHQ_P2', 'AFHQ_P2', 'Flower_P2', 'Cub_P2', 'Metface_P2')


def preset(args):
    """define_argparser.py:138-249 for the unconditional branch."""
    if args.seed == 0:
        args.seed = int(torch.randint(2**32, ()))
    seed_everything(args.seed)
    # routing by model name, define_argparser.py:147-165
    args.is_stable_diffusion = 'stable-diffusion' in args.model_name
    args.is_DeepFloyd_IF_diffusion = (not args.is_stable_diffusion) and 'DeepFloyd' in args.model_name
    args.is_LCM = (not args.is_stable_diffusion) and (not args.is_DeepFloyd_IF_diffusion) and 'LCM' in args.model_name
    if args.is_LCM:
        if not getattr(args, 'lcm_timesteps', None):
            # the two published rules give different timestep tables, and the shipped scripts edit at one of the entries that
            # differ (--num_inference_steps 4 --edit_t_idx 2: t = 499 against 519): a drop-in cannot choose silently
            raise NotImplementedError('the latent-consistency path (loco_edit_amd.tloco_lcm, edit.py:42-481) needs '
                                      '--lcm_timesteps {linspace,stride}: the reference pins no diffusers version that has '
                                      'LCMScheduler, and its two published set_timesteps rules differ -- linspace (current '
                                      'diffusers) gives [999, 759, 499, 259] for 4 steps, stride (as first released) '
                                      '[999, 759, 519, 279]')
        return _preset_t2i(args, 'LCM')
    if args.is_stable_diffusion:
        return _preset_t2i(args, 'Stable_Diffusion')
    if args.is_DeepFloyd_IF_diffusion:
        return _preset_t2i(args, 'DeepFloyd-IF')
    # model-name gate of define_argparser.py:166-176 (`unet_config` = an explicit architecture, tests / tiny configs)
    if getattr(args, 'unet_config', None) is None:
        if args.model_name == 'CelebA_HQ':
            raise NotImplementedError('Model weight deprecated...')
        if args.model_name in ('LSUN_bedroom', 'LSUN_cat', 'LSUN_horse'):
            raise NotImplementedError('Please download P2 weight from https://github.com/jychoi118/P2-weighting')
        if args.model_name not in UNCOND_MODELS_HF + UNCOND_MODELS_P2:
            raise ValueError('model_name choice: [CelebA_HQ_HF, LSUN_church_HF, FFHQ_HF]')
    args.exp = f'{args.model_name}-{args.dataset_name}'
    args.exp_folder = os.path.join(args.result_folder, args.exp)
    os.makedirs(args.exp_folder, exist_ok=True)
    # run-dir snapshot of the launching script (define_argparser.py:191-194), when it exists
    sh = os.path.join('scripts', args.sh_file_name)
    if args.sh_file_name and os.path.exists(sh):
        shutil.copy(sh, os.path.join(args.exp_folder, args.sh_file_name))
    args.obs_folder = os.path.join(args.exp_folder, 'obs')
    args.result_folder = os.path.join(args.exp_folder, 'results')
    os.makedirs(args.obs_folder, exist_ok=True)
    os.makedirs(args.result_folder, exist_ok=True)
    args.device = torch.device(args.device)
    args.dtype = torch.float32 if args.dtype == 'fp32' else torch.float16
    print(f'device : {args.device}, dtype : {args.dtype}')
    args.c_in = 3
    args.image_size = 256 if getattr(args, 'unet_config', None) is None else args.unet_config.resolution
    args.memory_bound = 50
    args.noise_schedule = 'linear'
    # asserts of define_argparser.py:245-247
    assert args.use_yh_custom_scheduler
    assert args.for_steps == 100
    assert args.performance_boosting_t == 0.2
    return args


def _preset_t2i(args, family):
    """define_argparser.py:147-160, 212-223, 236-239 for the text-to-image branches: Stable Diffusion (latent T-LOCO,
    c_in 4, image_size 64) and DeepFloyd-IF (pixel-space T-LOCO, c_in 3, image_size 64)."""
    args.exp = f'{family}-{args.dataset_name}-{args.note}'
    args.exp_folder = os.path.join(args.result_folder, args.exp)
    os.makedirs(args.exp_folder, exist_ok=True)
    sh = os.path.join('scripts', args.sh_file_name)
    if args.sh_file_name and os.path.exists(sh):
        shutil.copy(sh, os.path.join(args.exp_folder, args.sh_file_name))
    args.obs_folder = os.path.join(args.exp_folder, 'obs')
    args.result_folder = os.path.join(args.exp_folder, 'results')
    os.makedirs(args.obs_folder, exist_ok=True)
    os.makedirs(args.result_folder, exist_ok=True)
    args.device = torch.device(args.device)
    args.dtype = torch.float32 if args.dtype == 'fp32' else torch.float16
    print(f'device : {args.device}, dtype : {args.dtype}')
    from . import config
    if getattr(args, 'is_LCM', False):
        # SimianLuo/LCM_Dreamshaper_v7: the SD v1 denoiser with the guidance-scale embedding, the SD autoencoder's decoder; none of
        # the Stable Diffusion asserts below (define_argparser.py:242-243 of the reference: `elif args.is_LCM: pass`)
        if getattr(args, 'unet_config', None) is None:
            args.unet_config = config.LCM_DREAMSHAPER_V7_UNET
        if getattr(args, 'vae_config', None) is None:
            args.vae_config = config.SD_VAE_DECODER
        args.c_in = args.unet_config.in_channels
        args.image_size = args.unet_config.resolution
        args.memory_bound = 5
        return args
    if args.is_stable_diffusion:
        if getattr(args, 'unet_config', None) is None:
            # the Stable Diffusion v1.x denoiser (latent-diffusion UNetModel with SpatialTransformer blocks, 859.5 M
            # parameters; BASELINE config 4).  `--unet_preset sd64_xattn_standin` selects the round-2 stand-in
            # model names of the 2.x family (the shipped scripts: stabilityai/stable-diffusion-2-1-base) get that family's
            # widths: 1024-wide prompt states, 64-channel heads, nn.Linear proj_in / proj_out (config.SD21_BASE_UNET)
            args.unet_config = config.SD21_BASE_UNET if 'stable-diffusion-2' in args.model_name else config.SD15_UNET
        if getattr(args, 'vae_config', None) is None:
            args.vae_config = config.SD_VAE_DECODER
        if getattr(args, 'vae_encoder_config', None) is None:      # vae.encode of run_DDIMinversion (engine created on use)
            args.vae_encoder_config = config.SD_VAE_ENCODER
        if getattr(args, 'dataset', None) is None and args.dataset_name != 'Random':
            # the image datasets of the latent path are read at the autoencoder's resolution (utils.py:479-486: 512)
            from .utils import FolderDataset, SyntheticDataset
            r = args.vae_encoder_config.resolution
            args.dataset = (SyntheticDataset(r, 3) if args.dataset_name == 'Synthetic'
                            else FolderDataset(args.dataset_root, res=r, numeric=args.dataset_name != 'AFHQ'))
        if getattr(args, 'null_text_inversion', False):
            from .null_text import check_steps
            check_steps(args.inv_steps, args.for_steps)
        args.c_in = args.unet_config.in_channels           # 4
    else:
        if getattr(args, 'unet_config', None) is None:
            # the stage-I U-Net of the id the shipped scripts name (scripts/main_T2I_DeepFloydIF_null_space_projection*.sh:4,
            # DeepFloyd/IF-I-M-v1.0); `--unet_preset if64_standin` / `if64_xattn_standin` select the round-2 / 3 stand-ins
            parts = args.model_name.split("-")               # "DeepFloyd/IF-I-M-v1.0" -> size "M" (edit.py:1204)
            size = parts[2] if len(parts) > 2 and parts[2] in config.IF_I_WIDTH else "M"
            if size == "XL" and os.environ.get("LOCO_CFG_FORK", "1") == "0":
                # 4.3 B parameters x six device layouts (24 bytes per parameter) = 103 GB per independently loaded context: three of
                # them do not fit one GPU.  With the default shared parameter store (loco_fork: the guidance branches are forks of
                # one loaded context, round 6) the flow holds the parameters once -- ~103 GB + three arenas; not run at size here
                raise SystemExit("DeepFloyd/IF-I-XL-v1.0: three independently loaded contexts (LOCO_CFG_FORK=0) of the 4.3 B-parameter "
                                 "stage-I U-Net exceed one GPU's memory; leave LOCO_CFG_FORK at its default (one shared parameter store)")
            args.unet_config = config.if_stage1_config(size)
        args.c_in = 3
    args.image_size = args.unet_config.resolution          # 64: SD latents and the IF stage-I models alike
    args.memory_bound = 5
    assert args.use_yh_custom_scheduler
    assert args.performance_boosting_t <= 0
    return args


def seed_everything(seed: int):
    """define_argparser.py:251-258."""
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed % (2**32))
    random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
