"""A 200x200x130 scene with 100 proposals and one frame, run through the heatmap CLI (for a rocprofv3 kernel trace)."""
import json, os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.getcwd())
from nerf_rpn_amd.scripts import render_heatmap as R

root = tempfile.mkdtemp()
rng = np.random.default_rng(1)
for d in ("feat", "props", "ds/s0/train", "ds/s0/val"):
    os.makedirs(os.path.join(root, d))
shape = (200, 200, 130)
np.savez(os.path.join(root, "feat/s0.npz"), rgbsigma=np.zeros(shape + (4,), np.float32), resolution=np.array([130, 200, 200]))
c = rng.uniform(0, 1, (100, 3)) * shape
s = rng.uniform(10, 60, (100, 3))
np.savez(os.path.join(root, "props/s0.npz"), proposals=np.concatenate([c, s, rng.uniform(-1, 1, (100, 1))], 1).astype(np.float32))
json.dump({"room_bbox": [[0, 0, 0], [8, 8, 5.2]]}, open(os.path.join(root, "ds/s0/train/transforms.json"), "w"))
m = np.eye(4); m[:3, 3] = [1.0, 1.0, 2.0]
m[:3, :3] = np.array([[0.7071, 0, -0.7071], [-0.7071, 0, -0.7071], [0, 1, 0]])  # looking along +x+y, level
json.dump({"fl_x": 500, "fl_y": 500, "cx": 320, "cy": 240, "frames": [{"file_path": "images/0000.jpg", "transform_matrix": m.tolist()}]},
          open(os.path.join(root, "ds/s0/val/val_transforms.json"), "w"))
args = ["--dataset_dir", root + "/ds", "--feature_dir", root + "/feat", "--proposal_dir", root + "/props", "--output_dir", root + "/out"]
for k in range(3):
    t = time.perf_counter()
    R.main(args)
    print(f"run {k}: {1e3 * (time.perf_counter() - t):.1f} ms wall (host load + GPU + PNG write)")
