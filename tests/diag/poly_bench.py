"""Per-launch times of the up / down-sampling conv shapes of the CelebA-HQ DDPM network through loco_bench_conv (diagnostics build,
5 probes, 300 launches per number, three numbers per shape), on the route LOCO_POLYPHASE selects (read once per process: run it
twice).  LOCO_BENCH_GEOM picks the form: 1 nearest-x2 input, 2 zero-inserted input (pad 2), 4 conv + 2x2 sum-pool as one polyphase
launch (its 3x3 route is the plain launch below plus launch_pool2x2_sum).

    LOCO_HIP_LIB=loco-edit_amd/libloco_hip_diag.so LOCO_POLYPHASE=1 python3 tests/diag/poly_bench.py out.json
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import loco_edit_amd  # noqa
import loco_edit_amd.hip as H
from loco_edit_amd.config import CELEBA_DDPM, synth_params
eng = H.LocoEngine(CELEBA_DDPM, max_batch=10)
eng.load_state_dict(synth_params(CELEBA_DDPM, 0))
res = {}
for prec in ("bf16x3", "f16"):
    eng.set_precision(prec)
    for name, geom, c, hw in (("up 128->128 @256^2", 1, 128, 256), ("up 256->256 @128^2", 1, 256, 128),
                              ("zins 128->128 @256^2", 2, 128, 256), ("zins 128->128 @128^2", 2, 128, 128),
                              ("plain 3x3 128->128 @256^2", 0, 128, 256), ("plain 3x3 256->256 @128^2", 0, 256, 128),
                              ("conv+pool 128->128 @256^2 in", 4, 128, 256), ("conv+pool 256->256 @128^2 in", 4, 256, 128)):
        os.environ["LOCO_BENCH_GEOM"] = str(geom)
        for acc in ((0, 1) if geom == 2 else (0,)):
            os.environ["LOCO_BENCH_ACC"] = str(acc)
            try:
                ms = [eng.bench_conv(c, c, hw, hw, 5, 0, taps=9, iters=300) for _ in range(3)]
            except RuntimeError as e:
                print(prec, name, "n/a:", str(e)[:80], flush=True)
                continue
            res[f"{prec} {name}{' acc' if acc else ''}"] = [round(1000 * m, 1) for m in ms]
            print(prec, name, "acc" if acc else "", [f"{1000 * m:.1f} us" for m in ms], flush=True)
json.dump(res, open(sys.argv[1], "w"), indent=1)
