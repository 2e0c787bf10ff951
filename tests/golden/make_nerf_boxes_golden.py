"""Writes tests/golden/nerf_boxes_bounds.json: per case, boxes and mode of tests/nerf_boxes_ref.py the rays left out, the share of
counted samples, the tiles that hold one and, per tensor, the float32 checker's deviation from the float64 checker and the bound the
GPU test computes from it.  With an MI355X the "seen" entry of every tensor is the device's error against the float64 checker (and
tiles_run what the device counted); without one the entries of the file that is there are kept.  The file is a record: the tests
compute their bounds at run time.

Run from the repository root: ``python tests/golden/make_nerf_boxes_golden.py [output path]``."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import nerf_boxes_ref as B  # noqa: E402


def main(argv):
    path = os.path.join(HERE, "nerf_boxes_bounds.json")
    old = json.load(open(path)).get("cases", {}) if os.path.exists(path) else {}
    device = torch.cuda.is_available()
    if device:
        import test_gpu_nerf_boxes as T
    out = {"factor": B.FACTOR, "undecided": B.UNDECIDED, "device": device or any("seen" in t for c in old.values() for t in c["tensors"].values()),
           "cases": {}}
    for name in B.NAMES:
        for which in B.BOXES:
            for mode in B.MODES:
                c, boxes, table, f32, f64, left = B.refs_of(name, which, mode)
                key, keep = f"{name}-{which}-{mode}", ~left
                got = T.run(c, boxes, mode) if device else None
                rec = {"boxes": len(table), "rays_left_out": int(left.sum()), "counted": float(f64["counted1"].mean()),
                       "tiles": [B.tiles_counted(f64["counted1"]), B.tiles_counted(f64["counted2"]) if "counted2" in f64 else 0],
                       "tiles_total": [B.tiles_total(c.n_rays, c.s1), 0 if c.plain else B.tiles_total(c.n_rays, c.s1)], "tensors": {}}
                if device:
                    rec["tiles_run"] = got["tiles_run"].tolist()
                elif "tiles_run" in old.get(key, {}):
                    rec["tiles_run"] = old[key]["tiles_run"]
                for k in B.TENSORS:
                    if k not in f64:
                        continue
                    bound, err = B.bound_of(f32, f64, k, keep)
                    rec["tensors"][k] = {"fp32_error": err, "bound": bound}
                    if device:
                        seen, same = B.error_of(got, f64, k, keep)
                        rec["tensors"][k].update(seen=seen, nan_positions_equal=same)
                    elif "seen" in old.get(key, {}).get("tensors", {}).get(k, {}):
                        rec["tensors"][k].update({x: old[key]["tensors"][k][x] for x in ("seen", "nan_positions_equal")})
                out["cases"][key] = rec
    path = argv[1] if len(argv) > 1 else path
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main(sys.argv)
