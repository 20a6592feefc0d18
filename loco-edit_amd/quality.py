"""Edit-quality scores of decoded frames on the HIP engine: did the edit change the masked region (``mmse_in``), did the
null-space projection leave the rest alone (``mmse_out``), did the result stay perceptually close to the original (``ssim``,
``lpips``).  The metrics are those of ``eval.py`` (``eval.ssim``, ``eval.masked_mse``, ``eval.lpips``); here they run on
``hip.LocoQualityEngine`` (``csrc/quality.hip``) over frames that are already on the device, before they are quantised.

No pretrained AlexNet or ``lpips`` heads are available offline: the LPIPS weights come from ``--lpips_weights`` and without
them a request for ``lpips`` raises.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence

import torch

from . import eval as _eval

QUALITY_METRICS = ("ssim", "mmse", "lpips")


def parse_metrics(spec) -> List[str]:
    """``'ssim,mmse'`` (or a sequence) -> the metrics in the order of QUALITY_METRICS; ``''`` -> []."""
    names = [s.strip() for s in spec.split(",")] if isinstance(spec, str) else list(spec or [])
    names = [s for s in names if s]
    bad = [s for s in names if s not in QUALITY_METRICS]
    if bad:
        raise ValueError(f"quality_metrics {', '.join(bad)}: a comma list drawn from {','.join(QUALITY_METRICS)}")
    return [m for m in QUALITY_METRICS if m in names]


def load_lpips_weights(path: str) -> Dict[str, torch.Tensor]:
    """The LPIPS state dict of ``path`` under the names of ``eval.lpips_weight_names()``.  ``path`` is one file that holds
    all of them, or ``"features_file,heads_file"``: two files merged -- a torchvision AlexNet state dict (``features.*``) and
    the ``lpips`` package's ``alex.pth`` (``lin*.model.1.weight``).  ``net.`` prefixes are accepted, other keys ignored, a
    missing key is refused (the key handling of ``eval._lpips_weights``)."""
    if not path:
        raise NotImplementedError("LPIPS needs the pretrained AlexNet + `lpips` head weights, which are not available offline: "
                                  "pass --lpips_weights (one state dict, or 'features_file,heads_file')")
    merged = {}
    for part in path.split(","):
        merged.update(torch.load(part.strip(), map_location="cpu"))
    w = _eval._lpips_weights(merged)
    return {k: torch.as_tensor(w[k]).detach().to(torch.float32) for k in _eval.lpips_weight_names()}


class QualityScorer:
    """``metrics`` (a comma list or a sequence drawn from ssim, mmse, lpips) of frames on ``device``.  ``lpips_weights``: a
    path for ``load_lpips_weights`` or a state dict; requesting ``lpips`` without it raises here, before any device work.  The
    engine is created at the first call, for that call's frame size and count, and grown when a later call needs more."""

    def __init__(self, device, metrics=QUALITY_METRICS, lpips_weights=None, engine=None):
        self.device = device
        self.metrics = parse_metrics(metrics)
        self.lpips_weights_path = lpips_weights if isinstance(lpips_weights, str) else ""
        self._weights = None
        if "lpips" in self.metrics:
            if isinstance(lpips_weights, str) or lpips_weights is None:
                self._weights = load_lpips_weights(lpips_weights or "")
            else:
                w = _eval._lpips_weights(dict(lpips_weights))
                self._weights = {k: w[k] for k in _eval.lpips_weight_names()}
        self._engine = engine

    def engine(self, n: int, H: int, W: int):
        e = self._engine
        if e is None or e.max_pairs < n or e.max_hw[0] < H or e.max_hw[1] < W:
            from .hip import LocoQualityEngine
            old = (e.max_pairs, *e.max_hw) if e is not None else (0, 0, 0)
            e = LocoQualityEngine(max_hw=(max(H, old[1]), max(W, old[2])), max_pairs=max(n, old[0]), device=self.device)
            if self._weights is not None:
                e.load_state_dict(self._weights)
            self._engine = e
        return e

    # one value per pair, on the device
    def ssim(self, a, b, data_range=None):
        return self.engine(a.shape[0], a.shape[-2], a.shape[-1]).ssim(a, b, data_range=data_range)

    def lpips(self, a, b, normalize=False):
        if self._weights is None and self._engine is None:
            raise NotImplementedError("this scorer was built without LPIPS weights")
        return self.engine(a.shape[0], a.shape[-2], a.shape[-1]).lpips(a, b, normalize=normalize)

    def masked_mse(self, a, b, mask):
        return self.engine(a.shape[0], a.shape[-2], a.shape[-1]).masked_mse(a, b, mask)

    def score(self, frames: torch.Tensor, original_index: int, mask: Optional[torch.Tensor] = None) -> List[dict]:
        """frames [n,3,H,W] fp32 in [0, 1] on the device -> one record per frame against frame ``original_index``: ``ssim``
        (data range 1.0), ``mmse_in`` (over ``mask``, boolean [3,H,W] or [H,W]) and ``mmse_out`` (over its complement; both
        None without a mask or where that region is empty), ``lpips``; only the requested metrics appear."""
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"frames must be [n,3,H,W], got {tuple(frames.shape)}")
        n = frames.shape[0]
        if not 0 <= int(original_index) < n:
            raise ValueError(f"original_index {original_index} outside the {n} frames")
        a = frames.to(torch.float32).contiguous()
        b = a[int(original_index)][None].expand_as(a).contiguous()
        cols: Dict[str, Sequence] = {}
        if "ssim" in self.metrics:
            cols["ssim"] = self.ssim(a, b, data_range=1.0).tolist()
        if "mmse" in self.metrics:
            cols["mmse_in"] = cols["mmse_out"] = [None] * n
            if mask is not None:
                m = torch.as_tensor(mask).to(torch.bool)
                m = (m if m.dim() == 3 else m[None]).expand(3, *a.shape[-2:])
                for key, region in (("mmse_in", m), ("mmse_out", ~m)):
                    if bool(region.any()):
                        cols[key] = self.masked_mse(a, b, region[None]).tolist()
        if "lpips" in self.metrics:
            cols["lpips"] = self.lpips(a, b, normalize=True).tolist()
        return [{k: (None if v[i] is None else float(v[i])) for k, v in cols.items()} for i in range(n)]

    def report(self, frames: torch.Tensor, original_index: int, mask=None, alphas=None, exp_name: str = "") -> dict:
        """The dict a driver writes as ``<name>_quality.json``: the metrics, the weights path, the walk's alphas and per frame
        its record (with its alpha) against the original."""
        recs = self.score(frames, original_index, mask)
        alphas = [None] * len(recs) if alphas is None else [float(a) for a in alphas]
        if len(alphas) != len(recs):
            raise ValueError(f"{len(recs)} frames, {len(alphas)} alphas")
        return {"metrics": list(self.metrics), "lpips_weights": self.lpips_weights_path, "exp_name": exp_name,
                "alphas": alphas, "original_index": int(original_index), "masked": mask is not None,
                "frames": [dict(alpha=a, **r) for a, r in zip(alphas, recs)]}

    def write(self, path: str, frames: torch.Tensor, original_index: int, mask=None, alphas=None, exp_name: str = "") -> dict:
        out = self.report(frames, original_index, mask=mask, alphas=alphas, exp_name=exp_name)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        return out


def scorer_from_args(args, device) -> Optional[QualityScorer]:
    """The scorer of ``--quality_metrics`` / ``--lpips_weights``, or None when the flag is empty.  ``lpips`` without weights
    raises here: the drivers call this at construction, before any solve."""
    metrics = parse_metrics(getattr(args, "quality_metrics", "") or "")
    if not metrics:
        return None
    weights = getattr(args, "lpips_weights", "") or ""
    if "lpips" in metrics and not weights:
        raise ValueError("--quality_metrics lpips needs --lpips_weights (AlexNet features + lpips heads: one state dict, or "
                         "'features_file,heads_file'); no pretrained weights are available offline")
    return QualityScorer(device, metrics, weights if "lpips" in metrics else None)
