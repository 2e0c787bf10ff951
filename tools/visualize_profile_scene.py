"""A 200x200x130 scene with four objectness levels and 10 OBBs, run through the PLY export CLI (for a rocprofv3 kernel trace).

Prints the wall time of each CLI call and, for the last one, the split into loading, GPU work and the file write."""
import os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import visualize_rpn_input as V

root = tempfile.mkdtemp()
rng = np.random.default_rng(1)
for d in ("feat", "boxes", "obj", "out"):
    os.makedirs(os.path.join(root, d))
shape = (200, 200, 130)
rgbsigma = rng.uniform(0, 1, shape + (4,)).astype(np.float32)
rgbsigma[..., 3] = rng.uniform(-4, 4, shape)           # about half of the voxels above the 0.01 alpha threshold
np.savez(os.path.join(root, "feat/s0.npz"), rgbsigma=rgbsigma, resolution=np.array(shape))
c = rng.uniform(0.2, 0.8, (10, 3)) * shape
np.save(os.path.join(root, "boxes/s0.npy"), np.concatenate([c, rng.uniform(10, 40, (10, 3)), rng.uniform(-1, 1, (10, 1))], 1).astype(np.float32))
np.savez(os.path.join(root, "obj/s0.npz"), **{str(k): rng.normal(-3, 2, tuple(int(v) for v in np.ceil(np.array(shape) / 2 ** (k + 2))))
                                                .astype(np.float32) for k in range(4)})
args = ["-o", root + "/out", "-f", root + "/feat", "-b", root + "/boxes", "--objectness_dir", root + "/obj"]
for k in range(3):
    t = time.perf_counter()
    V.main(args)
    print(f"run {k}: {1e3 * (time.perf_counter() - t):.1f} ms wall (host load + GPU + PLY write), "
          f"{os.path.getsize(root + '/out/s0.ply') / 1e6:.1f} MB")
# the split of one scene: load, upload + kernels + download, write
t0 = time.perf_counter()
res, rs = V.load_feature(root + "/feat/s0.npz")
lv = V.load_levels(root + "/obj/s0.npz")
t1 = time.perf_counter()
score = ops.objectness_grid([torch.from_numpy(a).cuda() for a in lv], res)
count, rows = ops.ply_points(torch.from_numpy(rs).cuda(), res, 0.01, score)
b = rows.cpu().numpy().tobytes()
t2 = time.perf_counter()
with open(root + "/out/split.ply", "wb") as f:
    f.write(b)
t3 = time.perf_counter()
print(f"split: load {1e3 * (t1 - t0):.1f} ms, GPU incl. upload/download {1e3 * (t2 - t1):.1f} ms, write {1e3 * (t3 - t2):.1f} ms "
      f"({count} points, {len(b) / 1e6:.1f} MB)")
