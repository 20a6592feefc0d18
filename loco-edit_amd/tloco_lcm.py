"""Text-supervised T-LOCO on a latent-consistency model (``SimianLuo/LCM_Dreamshaper_v7``) on the MI355X engine: the class
``EditLatentConsistency`` with the method names, argument order and file names of the reference
(``src/modules/edit.py:42-481``).

LCM-Dreamshaper is the Stable Diffusion v1 U-Net, autoencoder and CLIP encoder; what the path adds to ``tloco_sd``:

* the guidance scale enters the NETWORK: ``w_embedding = get_guidance_scale_embedding(guidance_scale - 1)`` goes through
  ``time_embedding.cond_proj`` into the time embedding (``LocoEngine.set_time_cond``, ``config.*.time_cond_proj_dim``), so one
  denoiser evaluation per prompt replaces the two or three classifier-free-guidance branches;
* the scheduler's consistency step (``LocoEngine.lcm_step``, ``csrc/lcm.hip``): boundary-condition scalings and noise
  re-injection;
* the Jacobian of the decoded consistency function on ONE denoiser context,

      x0_hat(z_t) = vae.decode( (c_skip z_t + c_out (z_t - sigma eps(z_t)) / sqrt(a_t)) / 0.18215 )            (edit.py:206-247)
      J = J_dec . (1 / 0.18215) [ (c_skip + c_out / sqrt(a_t)) I - (c_out sigma / sqrt(a_t)) J_eps ].

Unpinned: diffusers is not installed and the reference's requirements pin a diffusers version that predates ``LCMScheduler``;
the scheduler, the guidance-scale embedding and the ``timestep_cond`` input are restated from the published
``LCMScheduler`` / ``LatentConsistencyModelPipeline`` / ``UNet2DConditionModel``.  The two published ``set_timesteps`` rules
differ, so the run names one (``--lcm_timesteps``).  ``clip_sample`` / thresholding (off in the model's scheduler config),
``strength < 1`` and LCM-LoRA are not built.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import solver
from .hip import LocoEngine
from .mask_segmentation import wants_segmentation
from .tloco import BranchStreams
from .tloco_sd import LATENT_SCALE, EditStableDiffusion, LatentCFGJacobianOperator, SDScheduler
from .utils import save_image as _save_image

TIMESTEP_RULES = ("linspace", "stride")


def lcm_timesteps(num_inference_steps: int, rule: str, original_inference_steps: int = 50, num_train_timesteps: int = 1000):
    """The N sampling timesteps out of the ``original_inference_steps`` training ones ``arange(1, 51) * 20 - 1`` (descending).
    ``linspace`` (current diffusers): indexed at ``floor(linspace(0, 50, N, endpoint=False))``; ``stride`` (LCMScheduler as
    first released): ``origin[::-(50 // N)][:N]``."""
    if rule not in TIMESTEP_RULES:
        raise ValueError(f"timestep rule must be one of {TIMESTEP_RULES}, got {rule!r}")
    N = int(num_inference_steps)
    if not 1 <= N <= original_inference_steps:
        raise ValueError(f"num_inference_steps must be in [1, {original_inference_steps}], got {N}")
    k = num_train_timesteps // original_inference_steps
    origin = np.arange(1, original_inference_steps + 1) * k - 1
    if rule == "stride":
        return [int(v) for v in origin[::-(len(origin) // N)][:N]]
    idx = np.floor(np.linspace(0, len(origin), num=N, endpoint=False)).astype(np.int64)
    return [int(v) for v in origin[::-1][idx]]


class LCMScheduler(SDScheduler):
    """diffusers' ``LCMScheduler`` as ``EditLatentConsistency`` uses it (edit.py:66, 94, 135): the pipeline's alpha-bar table
    (``SDScheduler``'s: scaled_linear 0.00085 .. 0.012, float32), integer timesteps by ``lcm_timesteps``, the update on the
    engine (``loco_lcm_step``)."""

    def __init__(self, engine=None, rule: str = "linspace", original_inference_steps: int = 50, timestep_scaling: float = 10.0,
                 sigma_data: float = 0.5, final_alpha_cumprod: float = 1.0):
        super().__init__(engine=engine)
        if rule not in TIMESTEP_RULES:
            raise ValueError(f"timestep rule must be one of {TIMESTEP_RULES}, got {rule!r}")
        self.rule, self.original_inference_steps = rule, int(original_inference_steps)
        self.timestep_scaling, self.sigma_data = float(timestep_scaling), float(sigma_data)
        self.final_alpha_cumprod = float(final_alpha_cumprod)

    def set_timesteps(self, num_inferences, device=None, **kwargs):
        self.timesteps = torch.tensor(lcm_timesteps(num_inferences, self.rule, self.original_inference_steps), dtype=torch.long)
        self.timesteps_next = None

    def index_of(self, t) -> int:
        return self.timesteps.tolist().index(int(t))

    def alpha_at(self, t) -> float:
        return float(self.alphas_cumprod[int(t)])

    def scalings(self, t) -> Tuple[float, float]:
        """(c_skip, c_out) of the boundary condition at timestep t: float64, rounded once to float32."""
        s = float(int(t)) * self.timestep_scaling
        sd2 = self.sigma_data * self.sigma_data
        return float(np.float32(sd2 / (s * s + sd2))), float(np.float32(s / math.sqrt(s * s + sd2)))

    def step_coeffs(self, t):
        """(index, alpha-bar at t, alpha-bar at the previous timestep, last): the previous timestep is the next table entry;
        behind the last one the sample is the denoised one (alpha-bar ``final_alpha_cumprod``, no noise)."""
        i = self.index_of(t)
        last = i == len(self.timesteps) - 1
        at_prev = self.final_alpha_cumprod if last else self.alpha_at(self.timesteps[i + 1])
        return i, self.alpha_at(t), at_prev, last

    def step(self, eps, t, x, noise: Optional[torch.Tensor] = None, **kwargs):
        """-> (prev_sample, denoised).  Stateless: the index is looked up from ``t``.  (diffusers keeps an internal step index
        that advances with every call; the reference relies on ``set_timesteps`` resetting it before each use --
        edit.py:106, 149, 207 -- which is why ``get_x0`` may step at any timestep of the table.)"""
        _, at, at_prev, last = self.step_coeffs(t)
        c_skip, c_out = self.scalings(t)
        x = x.contiguous()
        if last:
            noise = None
        elif noise is None:
            noise = torch.randn(x.shape, device=x.device, dtype=x.dtype)      # randn_tensor(model_output.shape, device=...)
        else:
            noise = noise.to(x.device, torch.float32).contiguous()
        return self.engine.lcm_step(x, eps.contiguous(), at, at_prev, c_skip, c_out, noise)


def guidance_scale_embedding(w: float, dim: int) -> torch.Tensor:
    """``LatentConsistencyModelPipeline.get_guidance_scale_embedding`` for one scale, float32 on the host: [dim]."""
    w = torch.tensor(w).repeat(1).to(torch.float32) * 1000.0
    half = dim // 2
    emb = torch.log(torch.tensor(10000.0)) / (half - 1)
    emb = torch.exp(torch.arange(half, dtype=torch.float32) * -emb)
    emb = w[:, None] * emb[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
    if dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1))
    return emb[0].contiguous()


class LatentLCMJacobianOperator(LatentCFGJacobianOperator):
    """J and J^T of the decoded consistency function on one denoiser context: the latent operator of ``tloco_sd`` with the
    scalars a = (c_skip + c_out / sqrt(a_t)) / 0.18215, b = c_out sigma / (sqrt(a_t) 0.18215) and a single branch of weight 1
    (the guidance lives inside the network)."""

    def __init__(self, engine: LocoEngine, decoder: LocoEngine, z, t, at, c_skip, c_out, z0_scaled, mask):
        a32 = np.float32(at)
        sq, sigma = float(np.sqrt(a32)), float(np.sqrt(np.float32(1.0) - a32))
        ls = float(np.float32(LATENT_SCALE))
        scalars = ((float(c_skip) + float(c_out) / sq) / ls, float(c_out) * sigma / (sq * ls))
        super().__init__({"net": engine}, [("net", 1.0)], decoder, z, t, at, z0_scaled, mask, scalars=scalars)


class EditLatentConsistency(EditStableDiffusion):
    BRANCH_NAMES = ("for", "edit")      # the guidance is folded into the network: no `null` branch

    def __init__(self, args):
        P = args.unet_config.time_cond_proj_dim
        if P <= 0:
            raise ValueError("the latent-consistency path needs a denoiser with a guidance-scale embedding (time_cond_proj_dim > "
                             "0: config.LCM_DREAMSHAPER_V7_UNET, --unet_preset tiny_lcm)")
        rule = getattr(args, "lcm_timesteps", None)
        if rule not in TIMESTEP_RULES:
            raise ValueError(f"lcm_timesteps must be one of {TIMESTEP_RULES}, got {rule!r}")
        super().__init__(args)
        if self.branch_streams.enabled:
            # the two contexts hold two prompts, they never run side by side: each keeps the whole chip
            for eng in self.branches.values():
                eng.set_chip_share(1)
            self.branch_streams = BranchStreams(1, self.device)
        # edit.py:66, 93-97
        self.scheduler = LCMScheduler(engine=self.engine, rule=rule, **getattr(args, "lcm_scheduler_kwargs", {}))
        self.num_inference_steps = args.num_inference_steps
        self.scheduler.set_timesteps(self.num_inference_steps, device=self.device)
        self.edit_t_idx = args.edit_t_idx
        # edit.py:118-121: the same embedding on both contexts (per context, not per parameter store)
        self.w_embedding = guidance_scale_embedding(self.guidance_scale - 1, P).to(self.device)
        for eng in self.branches.values():
            eng.set_time_cond(self.w_embedding)
        print(f'scheduler : LCM, timesteps ({rule}) {self.scheduler.timesteps.tolist()}, edit at index {self.edit_t_idx}; '
              f'w = {self.guidance_scale - 1} -> timestep_cond[{P}]')

    def _result_suffix(self, args) -> str:
        return ""                        # edit.py:51: no model-size suffix

    # ------------------------------------------------------------------ prompts
    def _branch(self, prompt) -> LocoEngine:
        """The context that holds `prompt`: the run's for / edit strings own one each (their states come from the text encoder
        or the ``prompt_emb`` dict); another string is encoded (``--text_encoder_path``) and takes the edit context."""
        if torch.is_tensor(prompt):
            name, emb = ("edit" if prompt is self.edit_prompt_emb else "for"), prompt
        elif prompt == self.for_prompt:
            name, emb = "for", self.for_prompt_emb
        elif prompt == self.edit_prompt:
            name, emb = "edit", self.edit_prompt_emb
        else:
            name, emb = "edit", self._get_prompt_emb(prompt)
        self._bind(name, emb)
        return self.branches[name]

    def _eps(self, eng: LocoEngine, latents, t):
        mb = eng.max_batch
        if latents.shape[0] <= mb:
            return eng.unet_forward(latents, float(t))
        out = torch.empty_like(latents)
        for b0 in range(0, latents.shape[0], mb):
            eng.unet_forward(latents[b0:b0 + mb].contiguous(), float(t), out=out[b0:b0 + mb])
        return out

    def _scaled(self, z):
        return self.engine.lincomb([(float(np.float32(1.0) / np.float32(LATENT_SCALE)), z)])

    # ------------------------------------------------------------------ sampler (edit.py:102-203)
    @torch.no_grad()
    def run_LCMforward(self, zT, prompt, num_samples=1):
        print('start LCMforward')
        return self.LCMforwardsteps(zT, prompt, t_start_idx=0, t_end_idx=-1)

    @torch.no_grad()
    def LCMforwardsteps(self, zt, prompt, t_start_idx=0, t_end_idx=-1, noise=None):
        """edit.py:147-203.  Decodes the last step's ``denoised / 0.18215`` (not the latents: they differ on every step but the
        last).  ``noise`` [steps, B, C, H, W]: the re-injected noise per timestep index (tests; default: drawn per step)."""
        self.scheduler.set_timesteps(self.num_inference_steps, device=self.device)
        eng = self._branch(prompt)
        latents = zt.to(self.device, torch.float32).contiguous()
        denoised = None
        for t_idx, t in enumerate(self.scheduler.timesteps):
            if t_idx < t_start_idx:
                continue
            elif t_start_idx == t_idx:
                pass
            elif t_idx == t_end_idx:
                return latents, t, t_idx
            model_pred = self._eps(eng, latents, t)
            latents, denoised = self.scheduler.step(model_pred, t, latents, noise=None if noise is None else noise[t_idx])
        x0 = (self.decode(self._scaled(denoised)) / 2 + 0.5).clamp(0, 1)
        if self.sharder.is_main:
            _save_image(x0, os.path.join(self.result_folder, f'{self.EXP_NAME}.png'), nrow=x0.size(0))
        return latents, (x0 * 255).to(torch.uint8).permute(0, 2, 3, 1)

    # ------------------------------------------------------------------ x0 (edit.py:206-247)
    def _denoised(self, eng, zt, t):
        at = self.scheduler.alpha_at(t)
        c_skip, c_out = self.scheduler.scalings(t)
        _, den = self.engine.lcm_step(zt, self._eps(eng, zt, t), at, 1.0, c_skip, c_out, None, want_prev=False)
        return den, at, c_skip, c_out

    def get_x0(self, zt, prompt, t, t_idx, mask=None, flatten=False):
        self.scheduler.set_timesteps(self.num_inference_steps, device=self.device)
        eng = self._branch(prompt)
        zt = zt.to(self.device, torch.float32).contiguous()
        x0_hat = self.decode(self._scaled(self._denoised(eng, zt, t)[0]))
        if mask is not None:
            return x0_hat[:, mask.to(x0_hat.device)]
        if flatten:
            x0_hat = x0_hat.view(x0_hat.shape[0], -1)
        return x0_hat

    def _operator(self, zt, prompt, t, mask):
        eng = self._branch(prompt)
        zt = zt.to(self.device, torch.float32).contiguous()
        den, at, c_skip, c_out = self._denoised(eng, zt, t)
        return LatentLCMJacobianOperator(eng, self.vae_engine, zt, float(t), at, c_skip, c_out, self._scaled(den), mask)

    # ------------------------------------------------------------------ direction through the Jacobian (edit.py:250-280)
    @torch.no_grad()
    def get_delta_zt_via_grad(self, zt, t, t_idx, for_prompt, edit_prompt, mask=None):
        """Unit-norm J_edit^T (x0_hat[edit] - x0_hat[for]) restricted to the mask: the image difference goes through the VJP of
        the EDIT-prompt Jacobian (edit.py:270)."""
        x0 = self.get_x0(zt, for_prompt, t, t_idx)
        x1 = self.get_x0(zt, edit_prompt, t, t_idx)
        d = self.engine.lincomb([(1.0, x1.view(1, -1).contiguous()), (-1.0, x0.view(1, -1).contiguous())])
        opj = self._operator(zt, edit_prompt, t, mask)
        opj.check_mask()
        v_ = opj.vjp(d)                                   # the decoder's cotangent seed applies the mask
        return self.engine.null_project(v_, None)         # v_ / v_.norm(dim=1)

    # ------------------------------------------------------------------ solver (edit.py:283-369)
    def local_encoder_decoder_pullback_zt(self, zt, t, t_idx, for_prompt, op=None, block_idx=None, pca_rank=50, chunk_size=25,
                                          min_iter=10, max_iter=100, convergence_threshold=1e-3, mask=None, v0=None, verbose=True):
        n = self.engine.n
        if v0 is None:
            v0 = torch.randn(n, pca_rank, device=self.device, dtype=torch.float)          # edit.py:312
        V = v0.to(self.device, torch.float32).T.contiguous()
        self.engine.qr_rows_(V)                                                            # :313
        opj = self._operator(zt, for_prompt, t, mask)
        self.last_solver_info = {}              # solver.solve_basis: which solver ran; the Krylov solver's residuals
        U, s, V, self.last_n_iter = solver.solve_basis(opj, self.engine, V, min_iter, max_iter, convergence_threshold,
                                                       sharder=self.sharder, verbose=verbose, info=self.last_solver_info)
        opj.check_mask()
        u = opj.gather(U).T.contiguous()
        return u, s.sqrt(), V

    # ------------------------------------------------------------------ driver (edit.py:373-471)
    @torch.no_grad()
    def x_space_guidance_direct(self, zt, t_idx, vk, single_edit_step):
        """zt + scale * step * vk, broadcast over the leading dimension as the reference's sum is (edit.py:475-479)."""
        shape = torch.broadcast_shapes(zt.shape, vk.shape)
        return self.engine.lincomb([(1.0, zt.expand(shape).contiguous()),
                                    (self.x_space_guidance_scale * single_edit_step, vk.expand(shape).contiguous())])

    @torch.no_grad()
    def run_edit_null_space_projection_zt(self, op, block_idx, vis_num, mask_index=0, vis_num_pc=1, vis_vT=False, pca_rank=50,
                                          edit_prompt=None, null_space_projection=False, pca_rank_null=50, non_semantic=False):
        """edit.py:373-471.  -> what the last ``LCMforwardsteps`` returns, (latents, uint8 frames) (the reference returns None);
        no basis cache, as in the reference."""
        self._set_edit_prompt(edit_prompt)
        self.scheduler.set_timesteps(self.num_inference_steps, device=self.device)
        zT = self._zT()
        self.EXP_NAME = "original"
        segment = wants_segmentation(self.args) and not self._exists(os.path.join(self.result_folder, "mask/mask.pt"))
        x0 = None
        if self.sharder.agree(not os.path.exists(os.path.join(self.result_folder, "original.png"))) or segment:
            print("Generating images and creating masks......")
            _, x0 = self.run_LCMforward(zT, prompt=self.for_prompt)
        # masks at the size of the decoded sample (edit.py:392: resolution 512 at full size)
        masks = self._masks((lambda: x0[0].detach().cpu().numpy()) if segment else None, x0.shape[1] if segment else None)
        if self.sampling_mode:
            return None
        mask = masks[mask_index].squeeze(dim=0).repeat(3, 1, 1)
        zt, t, t_idx = self.LCMforwardsteps(zT, t_start_idx=0, t_end_idx=self.edit_t_idx, prompt=self.for_prompt)
        assert t_idx == self.edit_t_idx
        if self.use_sega:
            self.EXP_NAME = f'sega_{self.edit_t_idx}T-{op}-block_{block_idx}_pos-edit_prompt-{self.edit_prompt}'
            out = self.LCMforwardsteps(zt, t_start_idx=self.edit_t_idx, t_end_idx=-1, prompt=self.edit_prompt)
            if self.clip_scoring and not non_semantic:
                # no unedited frame comes back: zt decoded once more under the `for` prompt, after the edit (the sampler draws
                # its re-injected noise from the global generator: the edit's frames are those of a run without scores)
                _, x_orig = self._decoded_as("_clip_original", lambda: self.LCMforwardsteps(
                    zt, t_start_idx=self.edit_t_idx, t_end_idx=-1, prompt=self.for_prompt))
                self._score_clip(out[1], original_frame=x_orig)
            return out
        print('!!!RUN LOCAL PULLBACK!!!')
        if non_semantic:
            _, _, vT_modify = self.local_encoder_decoder_pullback_zt(
                zt, t, t_idx, self.for_prompt, op=op, block_idx=block_idx, pca_rank=pca_rank, chunk_size=5, min_iter=10,
                max_iter=50, convergence_threshold=1e-3, mask=mask)
        else:
            vT_modify = self.get_delta_zt_via_grad(zt.clone(), t, t_idx, self.for_prompt, self.edit_prompt, mask=mask)
        vT_null = None
        if null_space_projection:
            _, _, vT_null = self.local_encoder_decoder_pullback_zt(
                zt, t, t_idx, self.for_prompt, op=op, block_idx=block_idx, pca_rank=pca_rank_null, chunk_size=5, min_iter=10,
                max_iter=50, convergence_threshold=1e-3, mask=~mask)
            vT_null = vT_null[:pca_rank_null, :].contiguous()
        vT = self.engine.null_project(vT_modify.contiguous(), vT_null)      # project, then unit rows (edit.py:427-433)
        self.last_vT = vT
        original_zt = zt.clone()
        self.EXP_NAME = (f'Edit_zt-edit_{self.edit_t_idx}T-{op}-block_{block_idx}_pos-edit_prompt-{self.edit_prompt}_select_mask'
                         f'{mask_index}_null_space_projection_{null_space_projection}_null_space_rank_{pca_rank_null}')
        # the +- walk of edit.py:444-462 as written: with k > 1 rows in vT every step carries k frames (zt + vk broadcasts), and
        # the frames are picked out of their concatenation
        vk = vT.view(-1, *zT.shape[1:])
        zts = {}
        for direction in (1, -1):
            zt_list = [original_zt.clone()]
            for _ in range(self.x_space_guidance_num_step):
                zt_list.append(self.x_space_guidance_direct(zt_list[-1], t_idx=self.edit_t_idx, vk=vk,
                                                            single_edit_step=direction * self.x_space_guidance_edit_step))
            zc = torch.cat(zt_list, dim=0)
            zts[direction] = zc[[0, -1], :] if vis_num == 1 else zc[::(zc.size(0) // vis_num)]
        zb = torch.cat([(zts[-1].flip(dims=[0]))[:-1], zts[1]], dim=0).contiguous()
        out = self.LCMforwardsteps(zb, t_start_idx=self.edit_t_idx, t_end_idx=-1, prompt=self.for_prompt)
        if self.clip_scoring and not non_semantic:
            # one text-supervised direction: frame j of the walk sits at alpha = j scale step
            self._score_clip(out[1], alphas=self._walk_alphas(vis_num))
        if not non_semantic:
            self._score_quality(out[1], self._walk_alphas(vis_num), mask)       # (gates itself on --quality_metrics)
        return out

    # names of the Stable Diffusion class that do not exist on this one (edit.py:42-481)
    _classifer_free_guidance = None
    DDIMforwardsteps = None
    run_DDIMforward = None
    run_DDIMinversion = None
    run_edit_null_space_projection_zt_semantic = None
    mask_diffedit = None
    MaskedDDPMforwardsteps = None
    _prepare = None
    _solve_or_load = None
    _z0_scaled = None
