"""``EditUncondDiffusion``: the LOCO-Edit pipeline for unconditional DDPMs on the
MI355X engine, with the method names, argument meaning, file layout and
``--vT_path`` format of the reference class (``src/modules/edit.py:2034-2625``).

What changed underneath: the denoiser, its Jacobian products, the scheduler
update and the subspace algebra are HIP kernels; batches stay resident on the
GPU (no ``buffer_device='cpu'`` bounce, no ``empty_cache`` per step); the solver
is ``solver.local_basis``.  Defects of the reference that cannot run
(``vis_power_spectral_density`` undefined, edit.py:2603) are not reproduced.
"""
from __future__ import annotations

import os

import torch

from . import solver
from .dist import ProbeSharder
from .mask_segmentation import wants_segmentation
from .utils import get_custom_diffusion_model, get_custom_diffusion_scheduler, get_dataset
from .utils import save_image as _save_image


class EditUncondDiffusion(object):
    def __init__(self, args):
        # default setting (edit.py:2037-2043)
        self.buffer_device = getattr(args, "buffer_device", "cpu")   # accepted, unused: batches stay in HBM
        self.memory_bound = getattr(args, "memory_bound", 50)
        self.device = args.device
        self.dtype = args.dtype
        self.seed = args.seed
        if self.dtype != torch.float32:
            raise ValueError("the unconditional hot path keeps fp32 tensors (scripts/main_celeba_hf_null_space_projection.sh:7); "
                             "the conv arithmetic is chosen with --precision")
        # --quality_metrics: the scorer of the decoded frames (None when off); lpips without weights raises here, before any solve
        from .quality import scorer_from_args
        self.quality = scorer_from_args(args, self.device)

        # get model (edit.py:2046-2052)
        self.unet = get_custom_diffusion_model(args)
        self.engine = self.unet.engine
        print(f'engine : {self.engine.version()}, conv arithmetic : {self.engine.get_precision()}')
        self.scheduler = get_custom_diffusion_scheduler(args, engine=self.engine)
        self.model_name = args.model_name

        self.image_size = args.image_size
        self.c_in = 3

        self.dataset = get_dataset(args)
        self.dataset_name = args.dataset_name

        self.for_steps = args.for_steps
        self.inv_steps = args.inv_steps
        self.use_yh_custom_scheduler = args.use_yh_custom_scheduler

        self.edit_t = args.edit_t
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        # edit.py:2071-2073
        self.edit_t_idx = int((self.scheduler.timesteps - self.edit_t * 1000).abs().argmin())
        self.performance_boosting_t_idx = (
            int((self.scheduler.timesteps - args.performance_boosting_t * 1000).abs().argmin())
            if args.performance_boosting_t > 0 else 1000)
        print(f'performance_boosting_t_idx: {self.performance_boosting_t_idx}')

        self.use_x_space_guidance = getattr(args, "use_x_space_guidance", False)
        self.x_space_guidance_edit_step = args.x_space_guidance_edit_step
        self.x_space_guidance_scale = args.x_space_guidance_scale
        self.x_space_guidance_num_step = args.x_space_guidance_num_step

        # path (edit.py:2084-2087)
        if self.dataset_name == "Random":
            self.result_folder = os.path.join(args.result_folder, f"sample_seed{args.seed}")
        else:
            self.result_folder = os.path.join(args.result_folder, f"sample_idx{args.sample_idx}")
        os.makedirs(self.result_folder, exist_ok=True)
        self.obs_folder = getattr(args, "obs_folder", None)
        self.vT_path = args.vT_path
        self.vT1_path = args.vT1_path
        self.sharder = ProbeSharder("world")
        # the modify-space and null-space solves of one edit share their probe batches (solver.local_basis_pair);
        # LOCO_PAIR_SOLVES=0 runs them one after the other as the reference does
        self.pair_solves = os.environ.get("LOCO_PAIR_SOLVES", "1") != "0"
        # the edited frames of all directions are decoded as one batch (LOCO_BATCH_DECODE=0: one direction after the other)
        self.batch_decode = os.environ.get("LOCO_BATCH_DECODE", "1") != "0"
        self.EXP_NAME = "exp"
        self.args = args

    # ------------------------------------------------------------------ multi-rank file discipline
    # Under torchrun every rank runs the same flow; rank 0 alone writes, and branch decisions that depend on the
    # file system are rank 0's (ranks taking different branches would hang in the solver's all-gather).
    def _save_image(self, *a, **k):
        if self.sharder.is_main:
            _save_image(*a, **k)

    def _save(self, obj, path):
        if self.sharder.is_main:
            torch.save(obj, path)

    def _save_residuals(self, basis_path, info):
        """``<basis name>_residual.json`` next to a basis file the Krylov solver computed (solver.write_residuals)."""
        if self.sharder.is_main:
            solver.write_residuals(basis_path, info)

    def _exists(self, path):
        return self.sharder.agree(bool(path) and os.path.exists(path))

    def _load(self, path, **kw):
        """torch.load on rank 0, broadcast to the others (they may not see rank 0's freshly written file yet)."""
        if not self.sharder.active:
            return torch.load(path, **kw)
        obj = torch.load(path, **kw) if self.sharder.is_main else None
        return self.sharder.agree(obj if obj is None else obj.cpu())

    # ------------------------------------------------------------------ helpers
    def _step(self, xt, t, eta, noise=None):
        """unet + scheduler.step fused on the device (edit.py:2151-2160 / 2572-2581)."""
        idx = self.scheduler.index_of(t)
        t_next = self.scheduler.timesteps_next[idx]
        at, at_next = self.scheduler.alpha_at(t), self.scheduler.alpha_at(t_next)
        if eta != 0 and noise is None:
            noise = torch.randn_like(xt)
        mb = self.engine.max_batch
        if xt.shape[0] <= mb:
            return self.engine.ddim_step(xt.contiguous(), float(t), at, at_next, eta, noise)
        out = torch.empty_like(xt)
        for b0 in range(0, xt.shape[0], mb):
            sl = slice(b0, b0 + mb)
            out[sl] = self.engine.ddim_step(xt[sl].contiguous(), float(t), at, at_next, eta,
                                            None if noise is None else noise[sl].contiguous())
        return out

    # ------------------------------------------------------------------ loops
    @torch.no_grad()
    def run_DDIMforward(self, num_samples=5):
        print('start DDIMforward')
        self.EXP_NAME = 'DDIMforward'
        xT = torch.randn(num_samples, self.c_in, self.image_size, self.image_size, device=self.device, dtype=self.dtype)
        self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=-1, vis_psd=False)

    @torch.no_grad()
    def run_DDIMinversion(self, idx, x0=None):
        """edit.py:2117-2167: x0 -> xT by DDIM with ascending t; 98 of the 99 steps run."""
        print('start DDIMinversion')
        EXP_NAME = f'DDIMinversion-{self.dataset_name}_{idx}'
        if not self.use_yh_custom_scheduler:
            raise ValueError('please set use_yh_custom_scheduler = True')
        self.scheduler.set_timesteps(self.inv_steps, device=self.device, is_inversion=True)
        timesteps = self.scheduler.timesteps
        if x0 is None:
            x0 = self.dataset[idx]
        self._save_image((x0 / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, 'original.png'))
        xt = x0.to(self.device, dtype=self.dtype).contiguous()
        for i, t in enumerate(timesteps):
            if i == len(timesteps) - 1:
                break
            xt = self._step(xt, t, eta=0)
        self._save_image((xt / 2 + 0.5).clamp(0, 1), os.path.join(self.result_folder, f'xT-{EXP_NAME}.png'))
        return xt

    @torch.no_grad()
    def DDIMforwardsteps(self, xt, t_start_idx, t_end_idx, vis_psd=False, save_image=True, return_xt=True,
                         performance_boosting=False, noises=None):
        """edit.py:2508-2614.  ``noises`` (optional, {step index: tensor}) injects the
        eta=1 draws so decodes are reproducible in tests."""
        print('start DDIMforward')
        assert (t_start_idx < self.for_steps) & (t_end_idx <= self.for_steps)
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        timesteps = self.scheduler.timesteps
        xt = xt.to(device=self.device, dtype=self.dtype).contiguous()
        for i, t in enumerate(timesteps):
            if t_end_idx == i:
                print('t_end_idx : ', i)
                return xt, t, i
            elif i < t_start_idx:
                continue
            elif t_start_idx == i:
                print('t_start_idx : ', i)
            if performance_boosting & (self.performance_boosting_t_idx <= i) & \
                    (self.performance_boosting_t_idx != len(timesteps) - 1):
                eta = 1
            else:
                eta = 0
            nz = None if (noises is None or eta == 0) else noises[i].to(self.device)
            xt = self._step(xt, t, eta=eta, noise=nz)
        if save_image:
            image = (xt / 2 + 0.5).clamp(0, 1)
            self._save_image(image, os.path.join(self.result_folder, f'{self.EXP_NAME}.png'), nrow=image.size(0))
        if return_xt:
            return xt
        return

    # ------------------------------------------------------------------ x0 / eps
    def get_x0(self, t, x, mask=None):
        """edit.py:2369-2391."""
        et = self.unet(x, t)
        at = self.scheduler.alpha_at(t)
        _, P_xt = self.engine.sched_step(x.contiguous(), et, at, at, 0.0, None, want_x0=True)
        if mask is not None:
            P_xt = P_xt[:, mask.to(P_xt.device)]
        return P_xt

    def get_et(self, t, x, mask=None):
        """edit.py:2394-2403."""
        et = self.unet(x, t)
        if mask is not None:
            et = et[:, mask.to(et.device)]
        return et

    # ------------------------------------------------------------------ solver
    def local_encoder_decoder_pullback_xt(self, x, t, op=None, block_idx=None, pca_rank=50, chunk_size=25,
                                          min_iter=10, max_iter=100, convergence_threshold=1e-3, mask=None,
                                          noise=False, v0=None, verbose=True):
        """edit.py:2406-2504 -> (u [L,k], s [k], vT [k,n]).  ``op``/``block_idx``/``chunk_size``
        are accepted and ignored exactly as in the reference."""
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        at = self.scheduler.alpha_at(t)
        self.last_solver_info = {}              # which solver ran (LOCO_SOLVER / --solver); the Krylov solver's residuals
        u, s, vT, self.last_n_iter = solver.local_basis(
            self.engine, x, t, at, pca_rank, mask=mask, noise=noise, min_iter=min_iter, max_iter=max_iter,
            convergence_threshold=convergence_threshold, v0=v0, sharder=self.sharder, verbose=verbose,
            info=self.last_solver_info)
        return u, s, vT

    # h-space baselines of the reference's own denoiser class (models/ddpm/diffusion.py:484-707): Pullback (x_t -> h) and the
    # decoder Jacobians h -> eps / h -> x0 with x_t and the skips fixed.  Argument names as there; ``op`` / ``block_idx`` must
    # name the bottleneck ('mid', 0: the only tap the reference's get_h_to_e implements), ``chunk_size`` is accepted and ignored
    # (the engine chunks by its max_batch).  ``s`` is sigma of J, as local_encoder_decoder_pullback_xt returns it.
    def _h_pullback(self, target, x, t, op, block_idx, pca_rank, min_iter, max_iter, convergence_threshold, mask, noise, v0,
                    verbose):
        if op not in (None, 'mid') or block_idx not in (None, 0):
            raise NotImplementedError(f"h-space tap (op, block_idx) = ({op!r}, {block_idx!r}): only ('mid', 0) is built")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        at = self.scheduler.alpha_at(t)
        self.last_solver_info = {}
        u, s, vT, self.last_n_iter = solver.local_basis(
            self.engine, x, t, at, pca_rank, mask=mask, noise=noise, min_iter=min_iter, max_iter=max_iter,
            convergence_threshold=convergence_threshold, v0=v0, sharder=self.sharder, verbose=verbose,
            info=self.last_solver_info, target=target)      # (LOCO_SOLVER=krylov: refused by local_basis for these targets)
        return u, s, vT

    def local_encoder_pullback_xt(self, x=None, t=None, op=None, block_idx=None, pca_rank=16, chunk_size=25,
                                  min_iter=10, max_iter=100, convergence_threshold=1e-3, v0=None, verbose=True):
        """diffusion.py:484-556 -> (u [n_h, k] = (J V_prev)^T, s [k], vT [k, n]) for J = d h / d x_t."""
        return self._h_pullback("h_enc", x, t, op, block_idx, pca_rank, min_iter, max_iter, convergence_threshold, None, True, v0,
                                verbose)

    def local_decoder_pullback_xt(self, x=None, t=None, op=None, block_idx=None, pca_rank=50, chunk_size=10,
                                  min_iter=10, max_iter=100, convergence_threshold=1e-3, mask=None, v0=None, verbose=True):
        """diffusion.py:558-632 for J = d eps / d h -> (u, s, vT) with the reference's swapped names: ``u`` [n_h, k] are the
        h-space directions (the right singular rows, transposed), ``vT`` [k, n_out] the rows J V_prev (:631).  ``mask``
        (an extension) selects outputs: ``vT`` is then [k, L]."""
        eT, s, hT = self._h_pullback("h_dec", x, t, op, block_idx, pca_rank, min_iter, max_iter, convergence_threshold, mask, True,
                                     v0, verbose)
        return hT.T.contiguous(), s, eT.T.contiguous()

    def local_x0_decoder_pullback_xt(self, x=None, t=None, at=None, op=None, block_idx=None, pca_rank=50, chunk_size=10,
                                     num_chunk=None, min_iter=10, max_iter=100, convergence_threshold=1e-3, mask=None, v0=None,
                                     verbose=True):
        """diffusion.py:634-707 for J = d x0_hat / d h = -sqrt(1 - at) / sqrt(at) . d eps / d h; names as
        ``local_decoder_pullback_xt``.  ``at`` is the scheduler's alpha-bar at ``t`` (the argument is accepted for the
        reference's signature and must agree with it when given)."""
        if at is not None and abs(float(at) - float(self.scheduler.alpha_at(t))) > 1e-6:
            raise ValueError(f"at = {float(at)} is not the scheduler's alpha-bar at t ({float(self.scheduler.alpha_at(t))})")
        eT, s, hT = self._h_pullback("h_dec", x, t, op, block_idx, pca_rank, min_iter, max_iter, convergence_threshold, mask, False,
                                     v0, verbose)
        return hT.T.contiguous(), s, eT.T.contiguous()

    # h-space PCA baselines of the same class (models/ddpm/diffusion.py:347-482): the unsupervised h-space directions LOCO is
    # compared against.  The samples stay on the device (hip.LocoPca, csrc/pca.hip) instead of going to ``pca_device``.
    def _h_tap_only(self, op, block_idx):
        if op not in (None, 'mid') or block_idx not in (None, 0):
            raise NotImplementedError(f"h-space tap (op, block_idx) = ({op!r}, {block_idx!r}): only ('mid', 0) is built")

    def _pca_generator(self, generator):
        return generator if generator is not None else torch.Generator().manual_seed(int(self.seed) % (2 ** 63))

    @torch.no_grad()
    def inv_jac_xt(self, x=None, t=None, op=None, block_idx=None, u=None, perturb_h=1e-1):
        """diffusion.py:347-377 -> vT [k, n] for u [n_h, k] (or [n_h]: k = 1).  The reference differentiates
        ``|| h + perturb_h u - get_h(x) ||`` at the ``x`` where that difference is ``perturb_h u``: row i is
        ``-J^T u_i / (|J^T u_i| + 1e-6)`` with J = d h / d x_t -- the NEGATIVE pullback of u_i, and independent of
        ``perturb_h`` (accepted for the signature).  One encoder primal and one cotangent pass per row."""
        self._h_tap_only(op, block_idx)
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        u = u.to(device=self.device, dtype=torch.float32)
        rows = (u.reshape(1, -1) if u.dim() == 1 else u.T).contiguous()
        self.engine.pmp_primal(x, float(t), self.scheduler.alpha_at(t), None, tap="enc")
        g = self.engine.pmp_vjp(rows)
        return -g / (g.norm(dim=1, keepdim=True) + 1e-6)

    @torch.no_grad()
    def local_pca_xt(self, x=None, t=None, op=None, block_idx=None, memory_bound=5, num_pca_samples=50000, pca_rank=512,
                     pca_device='cpu', return_x_direction=True, perturb_h=1e-1, noise=None, generator=None):
        """diffusion.py:379-436 -> (u [n_h, q], s [q], vT [q, n] | None): PCA (niter = 2) of ``get_h(x + eps / (|eps| + 1e-6))``
        over ``num_pca_samples`` Gaussian draws.  ``s`` are the singular values of the centred sample matrix, as
        ``torch.pca_lowrank`` returns them.  ``memory_bound`` is accepted (the engine chunks by its ``max_batch``);
        ``pca_device`` is accepted and ignored: the samples never leave the device.  Extensions: ``noise`` [N, C, R, R] injects
        the draws, ``generator`` seeds the range finder (default: a CPU generator seeded with the run's seed)."""
        from . import hspace_pca
        self._h_tap_only(op, block_idx)
        n = int(num_pca_samples)
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if noise is not None and (noise.dim() != 4 or noise.shape[0] != n or tuple(noise.shape[1:]) != tuple(x.shape[1:])):
            raise ValueError(f"noise must be [{n}, {', '.join(str(v) for v in x.shape[1:])}], got {tuple(noise.shape)}")
        store = hspace_pca.LocoPca(n, self.engine.n_h, int(pca_rank), device=self.device)
        mb = self.engine.max_batch
        for b0 in range(0, n, mb):
            b = min(mb, n - b0)
            eps = (torch.randn(b, *x.shape[1:], device=self.device, dtype=torch.float32) if noise is None
                   else noise[b0:b0 + b].to(device=self.device, dtype=torch.float32))
            hspace_pca.sample_h(self.engine, x + hspace_pca.normalize_wrt_batch(eps), t, store)
        s, u, mean = hspace_pca.pca_lowrank_device(store, int(pca_rank), 2, self._pca_generator(generator), center=True)
        self.last_pca = {"mean": mean, "n_samples": n, "routes": store.routes()}
        vT = self.inv_jac_xt(x=x, t=t, op=op, block_idx=block_idx, u=u, perturb_h=perturb_h) if return_x_direction else None
        return u, s, vT

    @torch.no_grad()
    def global_pca_xt(self, x=None, t=None, op=None, block_idx=None, memory_bound=5, pca_rank=512, pca_device='cpu',
                      generator=None):
        """diffusion.py:438-482 -> (u [n_h, q], s [q]): PCA (niter = 5) of ``get_h`` over the rows of ``x`` [N, C, R, R] (x_t of N
        independent x_T).  ``memory_bound`` / ``pca_device`` / ``generator``: as ``local_pca_xt``."""
        from . import hspace_pca
        self._h_tap_only(op, block_idx)
        store = hspace_pca.sample_h(self.engine, x, t, q_max=int(pca_rank))
        s, u, mean = hspace_pca.pca_lowrank_device(store, int(pca_rank), 5, self._pca_generator(generator), center=True)
        self.last_pca = {"mean": mean, "n_samples": int(x.shape[0]), "routes": store.routes()}
        return u, s

    # ------------------------------------------------------------------ drivers
    @torch.no_grad()
    def run_edit_hspace_pca(self, idx, vis_num, vis_num_pc=5, pca_rank=50, kind='global', num_samples=1000, edit='h', scale=1.0,
                            op='mid', block_idx=0, use_mask=True, **kwargs):
        """--run_edit_hspace_pca: edits along the unsupervised h-space directions (not in the reference's CLI; its class has the
        three functions only).  ``kind`` 'global': PCA of h at ``edit_t`` over ``num_samples`` fresh x_T; 'local': around the
        inverted image's x_t.  The basis ``{u, s, mean, t, kind, n_samples}`` is saved next to the other basis files and reused
        when present.  ``edit`` 'h': every remaining step of the decode gets ``alpha scale s_k / sqrt(N - 1) u_k`` added to the
        bottleneck (all frames of a walk in one batch); 'x': ``vT = inv_jac_xt(u)`` and the x-space walk of
        ``run_edit_null_space_projection``.  Grids and quality scores as there.  The sampling runs on every rank alike (no
        sharding)."""
        from . import hspace_pca
        if kind not in ('global', 'local') or edit not in ('h', 'x'):
            raise ValueError(f"kind must be 'global' or 'local' and edit 'h' or 'x', got {kind!r}, {edit!r}")
        n_s, q = int(num_samples), int(pca_rank)
        if q < 1 or q > min(n_s - 1, self.engine.n_h, hspace_pca.LocoPca.Q_LIMIT):
            raise ValueError(f"--hspace_pca_rank {q} must lie in [1, min(samples - 1, n_h, {hspace_pca.LocoPca.Q_LIMIT})] = "
                             f"[1, {min(n_s - 1, self.engine.n_h, hspace_pca.LocoPca.Q_LIMIT)}]")
        xT, mask = self._get_xT_and_mask(idx, use_mask)
        if xT is None:
            return None
        xt, t, t_idx = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=self.edit_t_idx)
        assert t_idx == self.edit_t_idx
        save_dir = os.path.join(self.result_folder, "basis", f'hspace_pca-{self.edit_t}T')
        os.makedirs(save_dir, exist_ok=True)
        basis_path = os.path.join(save_dir, f'hspace-pca-{kind}-rank-{q}-samples-{n_s}.pt')
        if self._exists(basis_path):
            print(f'loading the h-space PCA basis {basis_path}')
            basis = torch.load(basis_path, map_location="cpu") if self.sharder.is_main else None
            if self.sharder.active:
                basis = self.sharder.agree(basis)
            self.hspace_pca_reloaded = True
        else:
            self.hspace_pca_reloaded = False
            print(f'h-space PCA ({kind}): {n_s} samples of h at t = {int(t)}, rank {q}')
            gen = torch.Generator().manual_seed(int(self.seed) % (2 ** 63))
            if kind == 'global':
                shape = (self.c_in, self.image_size, self.image_size)
                mb = self.engine.max_batch
                store = hspace_pca.LocoPca(n_s, self.engine.n_h, q, device=self.device)
                for b0 in range(0, n_s, mb):
                    x_T = torch.randn(min(mb, n_s - b0), *shape, generator=gen).to(self.device)
                    x_t, _, _ = self.DDIMforwardsteps(x_T, t_start_idx=0, t_end_idx=self.edit_t_idx)
                    hspace_pca.sample_h(self.engine, x_t, t, store)
                s, u, mean = hspace_pca.pca_lowrank_device(store, q, 5, gen, center=True)
            else:
                u, s, _ = self.local_pca_xt(x=xt, t=t, op=op, block_idx=block_idx, num_pca_samples=n_s, pca_rank=q,
                                            return_x_direction=False, generator=gen,
                                            noise=torch.randn(n_s, *xt.shape[1:], generator=gen))
                mean = self.last_pca["mean"]
            basis = {"u": u.cpu(), "s": s.cpu(), "mean": mean.cpu(), "t": int(t), "kind": kind, "n_samples": n_s}
            self._save(basis, basis_path)
        u, s = basis["u"].to(self.device, torch.float32), basis["s"].to(self.device, torch.float32)
        n_pc = min(int(vis_num_pc), u.shape[1])
        alphas = self._walk_alphas(vis_num)
        BASIS_NAME = f"hspace-pca-{kind}-edit_{self.edit_t}T-{edit}-rank{q}-scale_{scale}"
        names = [f'{idx}-Edit-hspace_pca-{BASIS_NAME}-pc_{pc_idx:0=3d}' for pc_idx in range(n_pc)]
        original_xt = xt.detach()
        if edit == 'x':
            vT = self.inv_jac_xt(x=original_xt, t=t, op=op, block_idx=block_idx, u=u[:, :n_pc].contiguous())
            frames = [self.edit_batch(original_xt, vT[pc_idx, :], vis_num) for pc_idx in range(n_pc)]
            per = frames[0].shape[0]
            dec = self._decode_frames(torch.cat(frames, dim=0), n_pc, per)
        else:
            per = len(alphas)
            sigma = s[:n_pc] / float(basis["n_samples"] - 1) ** 0.5             # standard deviation of h along u_k
            a = torch.tensor(alphas, device=self.device, dtype=torch.float32)
            # dh [n_pc, per, n_h] = alpha_j scale sigma_k u_k
            dh = (float(scale) * sigma)[:, None, None] * a[None, :, None] * u[:, :n_pc].T[:, None, :]
            dec = hspace_pca.decode_with_dh(self, original_xt.expand(n_pc * per, -1, -1, -1), self.edit_t_idx,
                                            dh.reshape(n_pc * per, -1), performance_boosting=True)
        for pc_idx, name in enumerate(names):
            self.EXP_NAME = name
            image = (dec[pc_idx * per:(pc_idx + 1) * per] / 2 + 0.5).clamp(0, 1)
            self._save_image(image, os.path.join(self.result_folder, f'{name}.png'), nrow=image.size(0))
            self._score_quality(image, name, alphas, mask)
        return dec

    @torch.no_grad()
    def group_edit_null_space_projection(self, idx, **kwargs):
        """edit.py:2171-2212: compose two saved directions."""
        if self.dataset_name == 'Random':
            xT = torch.randn(1, 3, self.image_size, self.image_size, dtype=self.dtype, device=self.device)
        else:
            xT = self.run_DDIMinversion(idx=idx)
        xt, t, t_idx = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=self.edit_t_idx)
        assert t_idx == self.edit_t_idx
        print('loading the basis from --vT_path')
        vT_list = [self._load(self.vT_path), self._load(self.vT1_path)]
        BASIS_NAME = "load-basis-2"
        xt_temp = xt.detach().clone()
        xt_vis_list = [xt_temp]
        n = xt[0].numel()
        for pc_idx in range(2):
            vk = vT_list[pc_idx][0, :].to(self.device, torch.float32).contiguous()
            alpha = self.x_space_guidance_scale * self.x_space_guidance_num_step
            xt_edit = self.engine.edit_axpy(xt_temp.contiguous(), vk, [alpha])
            xt_temp = xt_edit
            xt_vis_list.append(xt_edit)
        self.EXP_NAME = f'{idx}-Edit_xt-noise-{BASIS_NAME}'
        xt_vis = torch.cat(xt_vis_list, dim=0)
        dec = self.DDIMforwardsteps(xt_vis, t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True)
        # frame 0 is the decoded unedited xt, the last one the composed edit; no mask on this path
        self._score_quality((dec / 2 + 0.5).clamp(0, 1), self.EXP_NAME, None, None, original_index=0)
        return xt

    def _segment(self, x0_fn):
        """SAM masks of the image `x0_fn()` ([1, 3, R, R] in [-1, 1]) at the model's resolution, cached as mask/mask.pt."""
        from .mask_segmentation import segment_for_driver

        def image():
            x0 = x0_fn()
            return ((x0 / 2 + 0.5).clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1)[0].detach().cpu().numpy()
        print("Creating masks......")
        return segment_for_driver(self.args, self.result_folder, self.sharder, image, self.image_size)

    def _get_xT_and_mask(self, idx, use_mask):
        """edit.py:2234-2267."""
        if self.dataset_name == 'Random':
            xT = torch.randn(1, self.c_in, self.image_size, self.image_size, dtype=self.dtype, device=self.device)
            mpath = os.path.join(self.result_folder, "mask/mask.pt")
            if wants_segmentation(self.args) and not self._exists(mpath):
                self.EXP_NAME = "original"                     # edit.py:2236-2241: sample, then segment the sample
                masks = self._segment(lambda: self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=-1))
            else:
                if not os.path.exists(mpath):
                    raise FileNotFoundError(
                        f"{mpath} missing: SAM mask generation is outside the hot path (SURVEY.md 2.1 #9); "
                        "provide mask.pt (bool [N,res,res])")
                masks = torch.load(mpath)
            if self.args.sampling_mode:
                return None, None
            mask = masks[self.args.mask_index].squeeze(dim=0).repeat(3, 1, 1)
            return xT, mask
        if self.dataset_name in ("CelebA_HQ_mask", "Synthetic"):
            xT = self.run_DDIMinversion(idx=idx)
            mask = self.dataset.getmask(idx=self.args.sample_idx, choose_sem=self.args.choose_sem)
            return xT, (mask if use_mask or self.dataset_name == "CelebA_HQ_mask" else None)
        # FFHQ / AFHQ / ... : SAM masks cached as mask/mask.pt, bool [N,res,res] (edit.py:2252-2267)
        mpath = os.path.join(self.result_folder, "mask/mask.pt")
        if wants_segmentation(self.args) and not self._exists(mpath):
            masks = self._segment(lambda: self.dataset[idx])    # edit.py:2253-2257: the dataset image
        else:
            if not os.path.exists(mpath):
                raise FileNotFoundError(
                    f"{mpath} missing: SAM mask generation is outside the hot path (SURVEY.md 2.1 #9); "
                    "provide mask.pt (bool [N,res,res]) as the reference's mask_segmentation.py writes it")
            print("loading masks")
            masks = torch.load(mpath)
        if self.args.sampling_mode:
            return None, None
        xT = self.run_DDIMinversion(idx=idx)
        mask = masks[self.args.mask_index].squeeze(dim=0).repeat(3, 1, 1) if use_mask else None
        return xT, mask

    @torch.no_grad()
    def run_edit_null_space_projection(self, idx, vis_num, vis_num_pc=5, pca_rank=50, pca_rank_null=10, op='mid',
                                       block_idx=0, null_space_projection=True, encoder_decoder_by_et=False,
                                       use_mask=True, random_edit=False, **kwargs):
        """edit.py:2216-2366."""
        xT, mask = self._get_xT_and_mask(idx, use_mask)
        if xT is None:
            return None
        # xT -> xt
        xt, t, t_idx = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=self.edit_t_idx)
        assert t_idx == self.edit_t_idx

        if not self._exists(self.vT_path):
            print('computing the local basis')
            tag = self.args.choose_sem if self.dataset_name in ("CelebA_HQ_mask", "Synthetic") else self.args.mask_index
            save_dir = os.path.join(self.result_folder, "basis", f'local_basis-{self.edit_t}T-select-mask-{tag}')
            os.makedirs(save_dir, exist_ok=True)
            # --jacobian_target h: the modify space is the Pullback basis (right singular rows of d h / d x_t, no mask); its
            # files carry a tag so that a cached x0 basis is never taken for it.  The null-space solve is the x0 one either way.
            hspace = getattr(self.args, "jacobian_target", "x0") == "h"
            htag = "-hspace" if hspace else ""
            vT_modify_path = os.path.join(save_dir, f'vT-modify-pca-rank-{pca_rank}{htag}.pt')
            vT_null_path = os.path.join(save_dir, f'vT-null-{pca_rank_null}.pt')

            vT_null = None
            have_m, have_n = self._exists(vT_modify_path), self._exists(vT_null_path)
            if null_space_projection and mask is not None and not have_m and not have_n and self.pair_solves and not hspace:
                # both bases are missing: one pass carries the probes of both solves (solver.local_basis_pair)
                print('subspace solves: modify space + null space (shared probe batches)')
                at = self.scheduler.alpha_at(t)
                pair_info = []
                (u_modify, s_modify, vT_modify, self.last_n_iter), (u_null, s_null, vT_null, self.last_n_iter_null) = \
                    solver.local_basis_pair(self.engine, xt.to(self.device, torch.float32), float(t), at, pca_rank, mask,
                                            pca_rank_null, ~mask, noise=encoder_decoder_by_et, min_iter=10, max_iter=50,
                                            convergence_threshold=1e-4, sharder=self.sharder, info=pair_info)
                self._save(vT_modify, vT_modify_path)
                self._save(vT_null, vT_null_path)
                if pair_info:
                    self._save_residuals(vT_modify_path, pair_info[0])
                    self._save_residuals(vT_null_path, pair_info[1])
            elif have_m:
                vT_modify = self._load(vT_modify_path, map_location=self.device).to(self.device).type(self.dtype)
            elif hspace:
                print('subspace solve: modify space (h-space pullback, d h / d x_t)')
                u_modify, s_modify, vT_modify = self.local_encoder_pullback_xt(
                    x=xt, t=t, op=op, block_idx=block_idx, pca_rank=pca_rank, min_iter=10, max_iter=50, convergence_threshold=1e-4)
                self._save(vT_modify, vT_modify_path)
            else:
                print('subspace solve: modify space')
                u_modify, s_modify, vT_modify = self.local_encoder_decoder_pullback_xt(
                    x=xt, t=t, op=op, block_idx=block_idx, pca_rank=pca_rank,
                    min_iter=10, max_iter=50, convergence_threshold=1e-4, mask=mask, noise=encoder_decoder_by_et)
                self._save(vT_modify, vT_modify_path)
                self._save_residuals(vT_modify_path, self.last_solver_info)

            if vT_null is not None:
                pass
            elif null_space_projection and self._exists(vT_null_path):
                vT_null = self._load(vT_null_path, map_location=self.device).to(self.device).type(self.dtype)
            elif null_space_projection:
                print('subspace solve: null space')
                u_null, s_null, vT_null = self.local_encoder_decoder_pullback_xt(
                    x=xt, t=t, op=op, block_idx=block_idx, pca_rank=pca_rank_null,
                    min_iter=10, max_iter=50, convergence_threshold=1e-4, mask=~mask, noise=encoder_decoder_by_et)
                self._save(vT_null, vT_null_path)
                self._save_residuals(vT_null_path, self.last_solver_info)

            if random_edit:
                vT_modify = torch.randn_like(vT_modify)       # same generator state on every rank (seed broadcast in main)

            # normalize vT (edit.py:2316-2323)
            if not null_space_projection:
                vT = self.engine.null_project(vT_modify.contiguous(), None)
            else:
                vT = self.engine.null_project(vT_modify.contiguous(), vT_null[:pca_rank_null, :].contiguous())
            BASIS_NAME = (f"{encoder_decoder_by_et}_{tag}-edit_{self.edit_t}T_null_proj_{null_space_projection}"
                          f"_rank{pca_rank_null}_scale_{self.x_space_guidance_scale}{htag}")
            # the reference loops range(max(vis_num_pc, vT.shape[0])) (edit.py:2329) and would raise
            # IndexError for vis_num_pc > rank; main.py always passes vis_num_pc == pca_rank
            for pc_idx in range(min(max(vis_num_pc, vT.shape[0]), vT.shape[0])):
                self.EXP_NAME = f'{idx}-Edit_xt-noise-{BASIS_NAME}-pc_{pc_idx:0=3d}'
                self._save(vT[[pc_idx], :], os.path.join(save_dir, f'{self.EXP_NAME}-vT.pt'))
        else:
            print('loading the basis from --vT_path')
            vT = self._load(self.vT_path).to(self.device, torch.float32)
            BASIS_NAME = f"edit_{self.edit_t}T-load-basis-'{os.path.basename(self.vT_path)}'"

        # edit (edit.py:2339-2364)
        original_xt = xt.detach()
        n_pc = min(vis_num_pc, vT.shape[0])
        names = [f'{idx}-Edit-random{random_edit}_xt-noise-{BASIS_NAME}-pc_{pc_idx:0=3d}' for pc_idx in range(n_pc)]
        if self.batch_decode and n_pc > 1:
            # the reference decodes one direction after the other (edit.py:2340-2364: vis_num_pc calls of
            # DDIMforwardsteps on 5 frames each); here the frames of ALL directions go through the 59 decode steps as one
            # batch (the denoiser runs 2.4x faster per frame at 25 frames than at 5), one image grid per direction
            # as before.  Only the assignment of the eta = 1 draws to frames differs (one draw per step for the batch).
            frames = [self.edit_batch(original_xt, vT[pc_idx, :], vis_num) for pc_idx in range(n_pc)]
            per = frames[0].shape[0]
            dec = self._decode_frames(torch.cat(frames, dim=0), n_pc, per)
            for pc_idx, name in enumerate(names):
                self.EXP_NAME = name
                image = (dec[pc_idx * per:(pc_idx + 1) * per] / 2 + 0.5).clamp(0, 1)
                self._save_image(image, os.path.join(self.result_folder, f'{name}.png'), nrow=image.size(0))
                self._score_quality(image, name, self._walk_alphas(vis_num), mask)
            return frames[-1]
        for pc_idx in range(n_pc):
            self.EXP_NAME = names[pc_idx]
            xt = self.edit_batch(original_xt, vT[pc_idx, :], vis_num)
            dec = self.DDIMforwardsteps(xt, t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True)
            self._score_quality((dec / 2 + 0.5).clamp(0, 1), names[pc_idx], self._walk_alphas(vis_num), mask)
        return xt

    @torch.no_grad()
    def run_edit_blended_diffusion(self, idx, edit_prompt, clip_guidance_scale=1000.0, num_aug=8, start_t=0.5, range_scale=50.0):
        """The Blended Diffusion baseline (blended.py): the text-driven edit of the source image inside the run's mask.  Writes
        <EXP_NAME>_blended.png (source | mask | result), <EXP_NAME>_clip.json (the scorer's numbers of the source and the result)
        and, with --quality_metrics, <EXP_NAME>_quality.json.  Returns the result [1, 3, H, W] in [-1, 1]."""
        import json
        from . import blended
        from .clip_score import load_clip
        from .define_argparser import check_blended_args
        check_blended_args(self.args, edit_prompt)
        xT, mask = self._get_xT_and_mask(idx, True)
        if xT is None:
            return None
        if mask is None:
            raise ValueError("Blended Diffusion edits inside a mask: this dataset / flag combination gave none")
        if self.dataset_name == 'Random':
            self.EXP_NAME = "original"
            x_src = self.DDIMforwardsteps(xT, t_start_idx=0, t_end_idx=-1)
        else:
            x_src = self.dataset[idx]
        x_src = x_src.to(self.device, torch.float32).reshape(1, self.c_in, self.image_size, self.image_size).clamp(-1, 1).contiguous()
        self.scheduler.set_timesteps(self.for_steps, device=self.device)
        scorer = load_clip(self.args.clip_model_path, tokenizer_path=getattr(self.args, "tokenizer_path", "") or None,
                           device=self.device, max_images=max(int(num_aug), 1), preprocess=getattr(self.args, "clip_preprocess", "device"),
                           grad=True)
        print(f"CLIP image tower: {scorer.vision.grad_bytes >> 20} MiB of records and workspace for the pixel gradient")
        text = scorer.text_embeds([edit_prompt])[0]
        tag = self.args.choose_sem if self.dataset_name in ("CelebA_HQ_mask", "Synthetic") else self.args.mask_index
        self.EXP_NAME = f'{idx}-Blended-mask_{tag}-start_{start_t}T-scale_{clip_guidance_scale}'
        out = blended.run(self.engine, self.scheduler, scorer, x_src, mask, text, self.seed, start_t,
                          clip_guidance_scale=clip_guidance_scale, range_scale=range_scale, num_aug=num_aug, verbose=True)
        image = (torch.cat([x_src, out]) / 2 + 0.5).clamp(0, 1)
        panel = torch.cat([image[:1], mask.to(self.device).float().view(1, self.c_in, self.image_size, self.image_size), image[1:]])
        self._save_image(panel, os.path.join(self.result_folder, f'{self.EXP_NAME}_blended.png'), nrow=3)
        if self.sharder.is_main:
            frames = (image * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            for_prompt = getattr(self.args, "for_prompt", "") or ""
            recs = scorer.score(frames, 0, for_prompt, edit_prompt)
            with open(os.path.join(self.result_folder, f"{self.EXP_NAME}_clip.json"), "w") as f:
                json.dump({"clip_model_path": self.args.clip_model_path, "clip_preprocess": scorer.preprocess_mode,
                           "for_prompt": for_prompt, "edit_prompt": edit_prompt, "exp_name": self.EXP_NAME,
                           "original": "the source image", "original_frame": recs[0], "frames": [dict(alpha=None, **recs[1])]}, f, indent=1)
        self._score_quality(image, self.EXP_NAME, None, mask, original_index=0)
        return out

    @torch.no_grad()
    def run_edit_asyrp(self, idx):
        """The Asyrp baseline (asyrp.py): a block f_t on the bottleneck, trained from the text pair --asyrp_src_prompt /
        --asyrp_tgt_prompt on the images --asyrp_train_idx (or loaded from --asyrp_ckpt when that file exists), then applied to
        image ``idx``: inversion, the asymmetric step from T to ``edit_t``, a plain decode below it.  Writes
        <EXP_NAME>_asyrp.png (the plain decode of the same x_T | the edit), <EXP_NAME>_clip.json, with --quality_metrics
        <EXP_NAME>_quality.json, and <EXP_NAME>_asyrp.json with the learning time and the transfer (edit) time.  Returns the
        edited image [1, 3, H, W] in [-1, 1]."""
        import json
        from . import asyrp, hspace_pca
        from .clip_score import load_clip
        from .define_argparser import check_asyrp_args
        from .hip import LocoAsyrpBlock
        args = self.args
        check_asyrp_args(args)
        if self.dataset is None:
            raise ValueError(f"--run_edit_asyrp trains on and edits dataset images: --dataset_name {self.dataset_name} has none")
        cfg = self.engine.cfg
        src, tgt = args.asyrp_src_prompt, args.asyrp_tgt_prompt
        scorer = load_clip(args.clip_model_path, tokenizer_path=getattr(args, "tokenizer_path", "") or None, device=self.device,
                           max_images=2, preprocess=getattr(args, "clip_preprocess", "device"), grad=True)
        text = scorer.text_embeds([src, tgt])
        Ch, Hh, Wh = self.engine.h_shape
        block = LocoAsyrpBlock(Ch, Hh, Wh, cfg.temb_ch, max_batch=1, gn_eps=cfg.gn_eps, seed=int(self.seed) % (2 ** 31), device=self.device)
        ckpt = args.asyrp_ckpt or os.path.join(self.result_folder, "asyrp_ckpt.pt")
        self.asyrp_trained = not self._exists(ckpt)
        learning_time, steps, mean_loss = 0.0, 0, None
        if self.asyrp_trained:
            train_idx = asyrp.parse_index_range(args.asyrp_train_idx)
            trainer = asyrp.AsyrpTrainer(self.engine, self.scheduler, scorer, block, text[0], text[1], cfg, lr=args.asyrp_lr,
                                         clip_weight=args.asyrp_clip_weight, rec_weight=args.asyrp_rec_weight)

            def learn():
                latents = {}
                loss = 0.0
                for epoch in range(int(args.asyrp_epochs)):
                    for i in train_idx:
                        if i not in latents:                 # the inversion is the same every epoch: kept on the host
                            latents[i] = self.run_DDIMinversion(idx=i).cpu()
                        self.scheduler.set_timesteps(self.for_steps, device=self.device)
                        loss = trainer.train_image(latents[i].to(self.device), self.edit_t_idx)
                        print(f"asyrp: epoch {epoch}, image {i}: mean loss {loss:.5f}")
                return loss
            mean_loss, learning_time = asyrp.timed(learn)
            steps = trainer.adam_step
            if self.sharder.is_main:
                asyrp.save_checkpoint(ckpt, block, steps, {"src_prompt": src, "tgt_prompt": tgt, "lr": args.asyrp_lr,
                                                           "epochs": int(args.asyrp_epochs), "train_idx": args.asyrp_train_idx})
        else:
            print(f"loading the Asyrp block {ckpt}")
            steps = asyrp.load_checkpoint(ckpt, block)
        xT = self.run_DDIMinversion(idx=idx)
        self.scheduler.set_timesteps(self.for_steps, device=self.device)

        def transfer():
            x_mid = asyrp.edit(self.engine, self.scheduler, block, cfg, xT, self.edit_t_idx, scale=args.asyrp_scale)
            return hspace_pca.decode_with_dh(self, x_mid, self.edit_t_idx, None)
        out, transfer_time = asyrp.timed(transfer)
        plain = hspace_pca.decode_with_dh(self, xT, 0, None)
        self.EXP_NAME = f'{idx}-Asyrp-edit_{self.edit_t}T-scale_{args.asyrp_scale}'
        image = (torch.cat([plain, out]) / 2 + 0.5).clamp(0, 1)
        self._save_image(image, os.path.join(self.result_folder, f'{self.EXP_NAME}_asyrp.png'), nrow=2)
        print(f"asyrp: learning time {learning_time:.2f} s ({steps} Adam steps), transfer edit time {transfer_time:.2f} s")
        if self.sharder.is_main:
            frames = (image * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            recs = scorer.score(frames, 0, src, tgt)
            with open(os.path.join(self.result_folder, f"{self.EXP_NAME}_clip.json"), "w") as f:
                json.dump({"clip_model_path": args.clip_model_path, "clip_preprocess": scorer.preprocess_mode, "for_prompt": src,
                           "edit_prompt": tgt, "exp_name": self.EXP_NAME, "original": "the plain decode of the inverted image",
                           "original_frame": recs[0], "frames": [dict(alpha=None, **recs[1])]}, f, indent=1)
            with open(os.path.join(self.result_folder, f"{self.EXP_NAME}_asyrp.json"), "w") as f:
                json.dump({"exp_name": self.EXP_NAME, "checkpoint": ckpt, "trained": bool(self.asyrp_trained), "adam_steps": int(steps),
                           "learning_time_s": learning_time, "transfer_edit_time_s": transfer_time, "final_mean_loss": mean_loss,
                           "src_prompt": src, "tgt_prompt": tgt, "lr": args.asyrp_lr, "epochs": int(args.asyrp_epochs),
                           "train_idx": args.asyrp_train_idx, "scale": args.asyrp_scale, "edit_t": self.edit_t}, f, indent=1)
        self._score_quality(image, self.EXP_NAME, None, None, original_index=0)
        return out

    def _score_quality(self, image, name, alphas, mask, original_index=None):
        """--quality_metrics: scores the decoded frames `image` [n,3,H,W] in [0, 1] (before they are quantised for the PNG) against
        the walk's alpha = 0 frame (or frame `original_index`) with quality.QualityScorer and writes
        <result_folder>/<name>_quality.json from the main rank.  Returns the JSON's dict (None off the main rank and without the flag)."""
        if getattr(self, "quality", None) is None or not self.sharder.is_main:
            return None
        if original_index is None:
            if 0.0 not in alphas:
                raise ValueError(f"walk alphas {alphas}: no unedited frame to score against")
            original_index = alphas.index(0.0)
        return self.quality.write(os.path.join(self.result_folder, f'{name}_quality.json'), image, original_index, mask=mask,
                                  alphas=alphas, exp_name=name)

    def _decode_frames(self, batch, n_pc, per):
        """Decode the frames of all directions (``n_pc`` walks of ``per`` frames) from the edit step to x0.

        The middle frame of every walk is the unedited ``xt`` itself (zero steps along the direction), i.e. the same
        image ``n_pc`` times.  Through the deterministic part of the decode (eta = 0: up to ``performance_boosting_t_idx``,
        edit.py:2556-2559) identical inputs stay identical, so only ONE copy goes through those steps; the copies are put
        back where the stochastic part starts (eta = 1: every frame then gets its own draw, as in the reference) or at the
        end.  ``LOCO_DEDUP_DECODE=0`` decodes all copies."""
        mid = per // 2
        dup = [d * per + mid for d in range(1, n_pc)]
        dedup = (os.environ.get("LOCO_DEDUP_DECODE", "1") != "0" and per % 2 == 1 and n_pc > 1
                 and all(torch.equal(batch[i], batch[mid]) for i in dup))
        n_t = len(self.scheduler.timesteps)
        pb = self.performance_boosting_t_idx
        stochastic = pb < n_t - 1                      # DDIMforwardsteps switches to eta = 1 from index pb on
        if not dedup or (stochastic and pb <= self.edit_t_idx):
            return self.DDIMforwardsteps(batch, t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True,
                                         save_image=False)
        keep = [i for i in range(batch.shape[0]) if i not in set(dup)]
        src = [keep.index(i) if i not in dup else keep.index(mid) for i in range(batch.shape[0])]     # full index -> unique index
        uniq = batch[keep].contiguous()
        if stochastic:
            uniq, _, _ = self.DDIMforwardsteps(uniq, t_start_idx=self.edit_t_idx, t_end_idx=pb, performance_boosting=True,
                                               save_image=False)
            return self.DDIMforwardsteps(uniq[src].contiguous(), t_start_idx=pb, t_end_idx=-1, performance_boosting=True,
                                         save_image=False)
        dec = self.DDIMforwardsteps(uniq, t_start_idx=self.edit_t_idx, t_end_idx=-1, performance_boosting=True,
                                    save_image=False)
        return dec[src].contiguous()

    def edit_batch(self, original_xt, vk_row, vis_num):
        """The +/- direction walk of edit.py:2346-2363 in one kernel: the S-fold
        repeated ``xt + scale*step*vk`` equals ``xt + j*scale*step*vk`` up to fp32
        rounding of the repeated adds; the reference's order of additions is kept by
        accumulating the scalar the same way."""
        return self.engine.edit_axpy(original_xt.contiguous(), vk_row.contiguous().view(-1), self._walk_alphas(vis_num))

    def _walk_alphas(self, vis_num):
        """The step sizes of the frames of one walk, the unedited frame (0) in the middle."""
        S = self.x_space_guidance_num_step
        stride = None if vis_num == 1 else (S + 1) // vis_num
        idxs = [0, S] if vis_num == 1 else list(range(0, S + 1, stride))
        step = self.x_space_guidance_scale * self.x_space_guidance_edit_step
        return [-j * step for j in reversed(idxs)][:-1] + [j * step for j in idxs]

    @torch.no_grad()
    def x_space_guidance_direct(self, xt, t_idx, vk, single_edit_step):
        """edit.py:2618-2625."""
        out = self.engine.edit_axpy(xt.contiguous(), vk.contiguous().view(-1),
                                    [self.x_space_guidance_scale * single_edit_step])
        return out
