"""One training step's ray stage of the reference's run_nerf.py (render_rays :514-614 at train time with given samples, the losses of
train :837-842) over the HIP operations: NeRF.query, ops.nerf_composite and ops.nerf_ray_losses (3.21).  Sample
drawing, ray batching, the loop and checkpoints are the caller's."""
import torch

from . import ops


def render_rays_train(model, rays_o, rays_d, viewdirs, z1, z2, embedded_cam, bb_center, bb_scale, noise=None):
    """render_rays for a batch of rays whose samples are given: z1 [S1] or [R, S1] non-decreasing, z2 [R, S2] in any order or None.

    model: a nerf_rpn_amd.NeRF; rays_o, rays_d, viewdirs [R, 3]; embedded_cam [input_ch_cam] or None; bb_center [3], bb_scale: the scene
    normalisation; noise [R, S1 + S2] or None: see ops.nerf_composite (its z2 columns follow the sorted z2).  The points are
    o + d z; z2 is sorted per ray before it is queried -- the query is pointwise, so this is the reference's sort after the
    concatenation (:507-510).  Returns the reference's dictionary: rgb_map, disp_map, acc_map, depth_map, z_vals, weights."""
    rays_o, rays_d = torch.as_tensor(rays_o, dtype=torch.float32), torch.as_tensor(rays_d, dtype=torch.float32)
    dev = next(model.parameters()).device
    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
    z1 = torch.as_tensor(z1, dtype=torch.float32).to(dev)

    def query(z):
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., :, None]
        return model.query(pts, viewdirs, embedded_cam, bb_center, bb_scale)
    raw1 = query(z1 if z1.dim() == 2 else z1[None, :].expand(rays_o.shape[0], -1))
    raw2 = None
    if z2 is not None:
        z2 = torch.sort(torch.as_tensor(z2, dtype=torch.float32).to(dev), -1).values
        raw2 = query(z2)
    rgb_map, disp_map, acc_map, weights, depth_map, z_vals = ops.nerf_composite(raw1, z1, rays_d, raw2, z2, noise)
    return {"rgb_map": rgb_map, "disp_map": disp_map, "acc_map": acc_map, "depth_map": depth_map, "z_vals": z_vals, "weights": weights}


def training_loss(out, target_s, target_d, target_vd, depth_loss_weight):
    """loss = img2mse(rgb_map, target_s) + depth_loss_weight * compute_depth_loss(...) (run_nerf.py:837-842) on render_rays_train's
    dictionary -> (loss, img_loss, depth_loss); without a positive depth_loss_weight the depth loss is not computed (None)."""
    if depth_loss_weight > 0.:
        img_loss, depth_loss = ops.nerf_ray_losses(out["rgb_map"], target_s, out["depth_map"], out["z_vals"], out["weights"], target_d,
                                                   target_vd)
        return img_loss + depth_loss_weight * depth_loss, img_loss, depth_loss
    img_loss, _ = ops.nerf_ray_losses(out["rgb_map"], target_s)
    return img_loss, img_loss, None
