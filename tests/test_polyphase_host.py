"""CPU: the folded operators of the polyphase up / down-sampling convs (loco-edit_amd/csrc/conv_plan.hip polyphase_fold, host code
only, dumped by tests/c/polyphase_fold_dump.cpp) against the identities they stand for, evaluated in float64 with torch on an
8 x 12 map:

  up conv            conv3x3_pad1(nearest2x(x))[2y+a][2x+b]  =  sum_{ty,tx} K[a][b][ty][tx] x[y+a-1+ty][x+b-1+tx]
  zero-insert dgrad  (sum_k w[k] z[Y-p+k], z[2u][2v] = g[u][v], p = 2 and 1)[2y+a][2x+b]  =  the same form on its own K

  conv + pool        pool2x2_sum(conv3x3_pad1(g))[y][x]  =  conv4x4_stride2_pad1(g), W4 = w (*) ones(2, 2)
                                                         =  sum_{p,q} sum_{ty,tx} K[p][q][ty][tx] g[2(y-p+ty)+p][2(x-q+tx)+q]

Off-image reads are zero.  K is a sum of at most four fp32 weights rounded ONCE to fp32, so with Kd the exact (float64) sums
  |K - Kd| <= 2^-24 |Kd|                                  (checked per entry)
  |out(K) - ref| <= 2^-24 sum |Kd| |x| + 64 * 2^-53 * A   (checked per output element; A = sum |w| |x|: float64 summation)
The zero-insert phases hold exactly 9 non-zero taps per (cout, cin) pair -- the 3x3 operator's own, each used once."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NIN, NOUT, H, W = 5, 64, 8, 12
KINDS = {"up": 0, "zins_pad2": 1, "zins_pad1": 2, "pool": 3}
OUT_KINDS = ["up", "zins_pad2", "zins_pad1"]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip(f"HIP headers not found under {ROCM}/include")
    tmp = tmp_path_factory.mktemp("polyphase")
    exe = str(tmp / "polyphase_fold_dump")
    cmd = [gxx, "-O2", "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
           os.path.join(ROOT, "loco-edit_amd", "csrc", "conv_plan.hip"), os.path.join(ROOT, "tests", "c", "polyphase_fold_dump.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    g = torch.Generator().manual_seed(11)
    w = (torch.randn(NOUT, NIN, 3, 3, generator=g) * 0.3 + 0.05).to(torch.float32)
    assert int((w == 0).sum()) == 0
    wpath = str(tmp / "w.f32")
    w.numpy().tofile(wpath)
    folded = {}
    for name, kind in KINDS.items():
        opath = str(tmp / f"{name}.f32")
        subprocess.run([exe, str(kind), str(NIN), str(NOUT), wpath, opath], check=True, timeout=60)
        k = np.fromfile(opath, dtype=np.float32).reshape(2, 2, 2, 2, NOUT, NIN)
        folded[name] = torch.from_numpy(k.copy())
    x = torch.randn(2, NIN, H, W, generator=g, dtype=torch.float64) + 0.5
    return w, folded, x


def _reference(name, w, x):
    """the 3x3 launch on the resampled map, float64 (the operator is a correlation, as the launch receives it)"""
    if name == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    p = 2 if name == "zins_pad2" else 1
    z = x.new_zeros(x.shape[0], x.shape[1], 2 * H, 2 * W)
    z[:, :, ::2, ::2] = x
    return F.conv2d(z, w, padding=p)[:, :, :2 * H, :2 * W]


def _exact_sums(name, w):
    """Kd[a][b][ty][tx][o][i] in float64 from the row / column tap sets of the identities"""
    sets = {"up": {0: ([0], [1, 2]), 1: ([0, 1], [2])},
            "zins_pad2": {0: ([0], [2]), 1: ([1], [])},
            "zins_pad1": {0: ([], [1]), 1: ([0], [2])}}[name]
    kd = torch.zeros(2, 2, 2, 2, NOUT, NIN, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for ty in range(2):
                for tx in range(2):
                    for ky in sets[a][ty]:
                        for kx in sets[b][tx]:
                            kd[a, b, ty, tx] += w[:, :, ky, kx].double()
    return kd


def _polyphase(k, x):
    """out[2y+a][2x+b] = sum K[a][b][ty][tx] xp[y+a+ty][x+b+tx], xp = x padded by one zero ring"""
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(x.shape[0], NOUT, 2 * H, 2 * W)
    for a in range(2):
        for b in range(2):
            kk = k[a, b].permute(2, 3, 0, 1).contiguous()      # [o][i][ty][tx]
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], kk)
    return out


@pytest.mark.parametrize("name", OUT_KINDS)
def test_folded_operator_is_the_identity_rounded_once(dump, name):
    w, folded, x = dump
    k, kd = folded[name].double(), _exact_sums(name, w)
    assert bool(((k - kd).abs() <= 2.0 ** -24 * kd.abs()).all()), "a folded weight is further than one fp32 rounding from its sum"
    ref = _reference(name, w.double(), x)
    # the identity itself, exact sums, float64
    assert float((_polyphase(kd, x) - ref).abs().max()) < 1e-12
    got = _polyphase(k, x)
    bound = 2.0 ** -24 * _polyphase(kd.abs(), x.abs()) + 64 * 2.0 ** -53 * _reference(name, w.double().abs(), x.abs())
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |out(K) - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["zins_pad2", "zins_pad1"])
def test_zero_insert_phases_hold_nine_taps(dump, name):
    w, folded, _ = dump
    nz = (folded[name] != 0).sum(dim=(0, 1, 2, 3))
    assert bool((nz == 9).all()), nz.unique()
    # ... and they are the operator's own nine values, each once
    vals = folded[name].permute(4, 5, 0, 1, 2, 3).reshape(NOUT, NIN, 16)
    got = torch.sort(vals.abs(), dim=2, descending=True).values[:, :, :9]
    want = torch.sort(w.reshape(NOUT, NIN, 9).abs(), dim=2, descending=True).values
    assert torch.equal(got, want)


def _pool_form(k, g):
    """sum over the four input phases of the 2x2 conv of the phase image, origin (-p, -q)"""
    hl, wl = g.shape[2] // 2, g.shape[3] // 2
    out = g.new_zeros(g.shape[0], NOUT, hl, wl)
    for p in range(2):
        for q in range(2):
            gp = F.pad(g[:, :, p::2, q::2], (1, 1, 1, 1))
            kk = k[p, q].permute(2, 3, 0, 1).contiguous()      # [o][i][ty][tx]
            out += F.conv2d(gp[:, :, 1 - p:1 - p + hl + 1, 1 - q:1 - q + wl + 1], kk)
    return out


def test_conv_then_pool_is_one_4x4_stride_2_conv(dump):
    w, folded, _ = dump
    g = torch.randn(2, NIN, 2 * H, 2 * W, generator=torch.Generator().manual_seed(5), dtype=torch.float64) + 0.5
    wd = w.double()
    ref = 4.0 * F.avg_pool2d(F.conv2d(g, wd, padding=1), 2)
    w4 = wd.new_zeros(NOUT, NIN, 4, 4)
    for a in range(2):
        for b in range(2):
            w4[:, :, a:a + 3, b:b + 3] += wd
    assert float((F.conv2d(g, w4, stride=2, padding=1) - ref).abs().max()) < 1e-12      # the identity itself
    # the folded taps are W4's, each rounded once: tap (ty, tx) of phase (p, q) is W4[2 ty + 1 - p][2 tx + 1 - q]
    k = folded["pool"].double()
    kd = torch.zeros_like(k)
    for p in range(2):
        for q in range(2):
            for ty in range(2):
                for tx in range(2):
                    kd[p, q, ty, tx] = w4[:, :, 2 * ty + 1 - p, 2 * tx + 1 - q]
    assert bool(((k - kd).abs() <= 2.0 ** -24 * kd.abs()).all())
    assert float((_pool_form(kd, g) - ref).abs().max()) < 1e-12
    bound = 2.0 ** -24 * _pool_form(kd.abs(), g.abs()) + 64 * 2.0 ** -53 * 4.0 * F.avg_pool2d(F.conv2d(g.abs(), wd.abs(), padding=1), 2)
    worst = float(((_pool_form(k, g) - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"pool: max |out(K) - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
