"""Training of the reference's run_nerf.py over the HIP operations: the ray stage of a step (render_rays :514-614 at train time, the
losses of train :837-842) through NeRF.query, ops.nerf_composite and ops.nerf_ray_losses (3.21); its front end (the
ray batch :650-670, the perturbed first list :480-495, the drawn second list :588-592) through ops.nerf_train_batch and
ops.nerf_train_samples (3.22); and the loop of train_nerf (:811-922) with its checkpoints.  Depth completion, tensorboard, the
``i_img`` images, LPIPS, N_importance > 0 and more than one GPU are not covered."""
import json
import os
import warnings
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .nerf_model import NeRF


def render_rays_train(model, rays_o, rays_d, viewdirs, z1, z2, embedded_cam, bb_center, bb_scale, noise=None, depth_range=None, u=None,
                      lower_bound=None, near=None, far=None):
    """render_rays for a batch of rays whose samples are given: z1 [S1] or [R, S1] non-decreasing, z2 [R, S2] in any order or None.

    model: a nerf_rpn_amd.NeRF; rays_o, rays_d, viewdirs [R, 3]; embedded_cam [input_ch_cam] or None; bb_center [3], bb_scale: the scene
    normalisation; noise [R, S1 + S2] or None: see ops.nerf_composite (its z2 columns follow the sorted z2).  The points are
    o + d z; z2 is sorted per ray before it is queried -- the query is pointwise, so this is the reference's sort after the
    concatenation (:507-510).  Returns the reference's dictionary: rgb_map, disp_map, acc_map, depth_map, z_vals, weights.

    z2 = "draw": the second list is drawn as the reference draws it at train time (:588-592) -- ops.nerf_train_samples on the first
    list's raw, detached, with depth_range [R, 3] or None, the uniforms u [R, S1] or None (deterministic), lower_bound, near and far --
    and the dictionary also holds it, unsorted, as "z_vals_2"."""
    rays_o, rays_d = torch.as_tensor(rays_o, dtype=torch.float32), torch.as_tensor(rays_d, dtype=torch.float32)
    dev = next(model.parameters()).device
    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
    z1 = torch.as_tensor(z1, dtype=torch.float32).to(dev)

    def query(z):
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., :, None]
        return model.query(pts, viewdirs, embedded_cam, bb_center, bb_scale)
    raw1 = query(z1 if z1.dim() == 2 else z1[None, :].expand(rays_o.shape[0], -1))
    raw2 = drawn = None
    if isinstance(z2, str):
        if z2 != "draw":
            raise ValueError(f"render_rays_train: z2 is a tensor, None or 'draw', got {z2!r}")
        if lower_bound is None or near is None or far is None:
            raise ValueError("render_rays_train: z2='draw' needs lower_bound, near and far")
        z2 = drawn = ops.nerf_train_samples(raw1.detach(), z1, torch.cat([rays_o, rays_d], -1), near, far, lower_bound, depth_range, u)
    if z2 is not None:
        z2 = torch.sort(torch.as_tensor(z2, dtype=torch.float32).to(dev), -1).values
        raw2 = query(z2)
    rgb_map, disp_map, acc_map, weights, depth_map, z_vals = ops.nerf_composite(raw1, z1, rays_d, raw2, z2, noise)
    out = {"rgb_map": rgb_map, "disp_map": disp_map, "acc_map": acc_map, "depth_map": depth_map, "z_vals": z_vals, "weights": weights}
    if drawn is not None:
        out["z_vals_2"] = drawn
    return out


def training_loss(out, target_s, target_d, target_vd, depth_loss_weight):
    """loss = img2mse(rgb_map, target_s) + depth_loss_weight * compute_depth_loss(...) (run_nerf.py:837-842) on render_rays_train's
    dictionary -> (loss, img_loss, depth_loss); without a positive depth_loss_weight the depth loss is not computed (None)."""
    if depth_loss_weight > 0.:
        img_loss, depth_loss = ops.nerf_ray_losses(out["rgb_map"], target_s, out["depth_map"], out["z_vals"], out["weights"], target_d,
                                                   target_vd)
        return img_loss + depth_loss_weight * depth_loss, img_loss, depth_loss
    img_loss, _ = ops.nerf_ray_losses(out["rgb_map"], target_s)
    return img_loss, img_loss, None


# ----------------------------------------------------------------------------------------------------------------------
# the loop (train_nerf :755-922)
# ----------------------------------------------------------------------------------------------------------------------
def learning_rate(i, lrate, start_decay, end_decay):
    """The rate in effect at step i (:819-823): lrate up to start_decay, lrate * 0.1 ** portion inside (start_decay, end_decay], and
    after end_decay the last value set, lrate * 0.1 ** 1."""
    if i <= start_decay:
        return lrate
    portion = (min(i, end_decay) - start_decay) / (end_decay - start_decay)
    return lrate * (0.1 ** portion)


def precompute_quadratic_samples(near, far, num_samples):
    """The fork's function as DESIGN.md 3.16 assumes it (scripts/nerf_render.py has the same), float32."""
    x = torch.linspace(0, 1, num_samples)
    a = (far - near) / (1. + 2. * 0.1)
    return a * x.pow(2) + 2. * 0.1 * a * x + near


def base_samples(args, near, far):
    """The list every ray's first samples start from, float32 on the host -> (z [S1], two_pass).  depth_loss_weight > 0: the
    N_samples // 2 precomputed quadratic samples, one fewer if that is odd (:1076-1080); else N_samples between near and far, linear
    in depth or in inverse depth, in render_rays' float32 expression on [1, 1] bounds (:571, :602-606)."""
    if args.depth_loss_weight > 0.:
        z = precompute_quadratic_samples(near, far, args.N_samples // 2)
        if z.shape[0] % 2 == 1:
            z = z[:-1]
        if z.shape[0] < 2:
            raise ValueError(f"nerf_train: N_samples {args.N_samples} leaves {z.shape[0]} precomputed samples, at least 2 are needed")
        return z.contiguous(), True
    t_vals = torch.linspace(0., 1., steps=int(args.N_samples))
    n_t, f_t = torch.full((1, 1), float(near)), torch.full((1, 1), float(far))
    z = n_t * (1. - t_vals) + f_t * t_vals if not args.lindisp else 1. / (1. / n_t * (1. - t_vals) + 1. / f_t * t_vals)
    return z.reshape(-1).contiguous(), False


def newest_checkpoint(run_dir):
    """The last ``.tar`` of a run's directory in sorted order (the names are zero-padded step numbers), or None."""
    names = sorted(n for n in os.listdir(run_dir) if n.endswith(".tar")) if os.path.isdir(run_dir) else []
    return os.path.join(run_dir, names[-1]) if names else None


def read_by_the_tools(name):
    """Whether scripts/nerf_extract.py's load_checkpoint, and so nerf_render, nerf_test and nerf_extract, consider a checkpoint of this
    name: the reference's rule (:335)."""
    return "000.tar" in name


def save_checkpoint(path, step, model, optimizer, embedcam):
    """The reference's dictionary (:854-857) -- the network's keys with ``module.`` as its DataParallel writes them -- plus the camera
    embedding, which the reference re-derives from its seed.  global_step is the number of steps done."""
    d = {"global_step": step, "network_fn_state_dict": {"module." + k: v.detach().cpu() for k, v in model.state_dict().items()},
         "optimizer_state_dict": optimizer.state_dict()}
    if embedcam is not None:
        d["embedcam_state_dict"] = {k: v.detach().cpu() for k, v in embedcam.state_dict().items()}
    torch.save(d, path)
    print("Saved checkpoints at", path)


def write_args(args):
    """run_nerf :1019-1025: ``<ckpt_dir>/<expname>/args.json``."""
    run_dir = os.path.join(args.ckpt_dir, args.expname)
    os.makedirs(run_dir, exist_ok=True)
    with open(os.path.join(run_dir, "args.json"), "w") as f:
        json.dump({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in vars(args).items()}, f, indent=4)
    return run_dir


def train(run, args, rand=None):
    """The loop of train_nerf (:811-922) on one GPU -> SimpleNamespace(model, optimizer, embedcam, step, log).

    run: images [N, H, W, 3], depths [N, H, W, 2] (depth, std) and valid_depths [N, H, W] (both None without a depth prior), poses
    [N, 4, 4], intrinsics [N, 4], near, far, bb_center [3], bb_scale -- the training views, float32 tensors that are moved to the
    device once; optionally state_dict (a network_fn_state_dict) and embedcam [N, input_ch_cam] to start from.  args: the flags of
    scripts/nerf_train.py; args.dtype ("fp32" when absent, or "bf16x3") is the arithmetic of the trunk in every query of a step, forward
    and backward; args.backward_dtype ("fp32" when absent, or "bf16x3" beside dtype "bf16x3") that of the backward's own products
    (DESIGN.md 3.24).  The seeds are the reference's (:756-758) -- the streams are not: torch's
    generator here is the device's Philox stream of this build, numpy's is numpy's.

    Per step: np.random.choice over the views, N_rand pixels without replacement (np.random.choice(H W, N_rand, replace=False), the
    assumed select_coordinates), ops.nerf_train_batch, render_rays_train, training_loss, backward, clip_grad_value_(0.1), Adam.  The
    camera embedding is created after the model and is not given to the optimiser, as in the reference (:807-809); a step therefore
    uses it detached.  Loss and PSNR are read from the device every i_print steps only; nothing else in a step synchronises.
    log: [(step, loss, img_loss, psnr)] of those reads.

    rand(step, name, shape) -> tensor / array or None: a hook that supplies a step's random numbers; name is "image" (the view's
    index), "pix" [N_rand], "t_rand" [N_rand, S1], "u" [N_rand, S1] or "noise" [N_rand, S1 + S2].  None falls back to the generators."""
    if not torch.cuda.is_available():
        raise ops.lib.NrpnError("nerf_train needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    np.random.seed(0)
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    # ops.nerf_grid_config raises for an option the kernels do not cover; args.dtype: the arithmetic of the trunk
    model = NeRF(dict(vars(args)), dtype=getattr(args, "dtype", "fp32"), backward_dtype=getattr(args, "backward_dtype", "fp32")).to(dev)
    params = list(model.parameters())
    optimizer = torch.optim.Adam(params=params, lr=args.lrate, betas=(0.9, 0.999))
    n_views = int(run.images.shape[0])
    cam_ch = ops.nerf_grid_config(model.cfg)["input_ch_cam"]
    embedcam = torch.nn.Embedding(n_views, cam_ch).to(dev) if cam_ch > 0 else None

    if getattr(run, "state_dict", None) is not None:         # start from these weights instead of torch's initialisation
        model.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in run.state_dict.items()})
    if embedcam is not None and getattr(run, "embedcam", None) is not None:
        with torch.no_grad():
            embedcam.weight.copy_(torch.as_tensor(run.embedcam, dtype=torch.float32))
    run_dir = os.path.join(args.ckpt_dir, args.expname)
    os.makedirs(run_dir, exist_ok=True)
    start = 0
    ckpt_path = None if args.no_reload else newest_checkpoint(run_dir)
    if ckpt_path is not None:
        print("Reloading from", ckpt_path)
        ckpt = torch.load(ckpt_path, map_location="cpu")
        start = int(ckpt["global_step"])
        model.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in ckpt["network_fn_state_dict"].items()})
        optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        if embedcam is not None and "embedcam_state_dict" in ckpt:
            embedcam.load_state_dict(ckpt["embedcam_state_dict"])

    def f32(x):
        return torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
    images, poses, intrinsics = f32(run.images), f32(run.poses), f32(run.intrinsics)
    H, W = int(images.shape[1]), int(images.shape[2])
    near, far = float(run.near), float(run.far)
    bb_center, bb_scale = f32(run.bb_center), f32(run.bb_scale)
    z, two_pass = base_samples(args, near, far)
    lower_bound = float(z[-1] - z[-2]) if two_pass else None      # render_rays :577, float32
    z = z.to(dev)
    S1 = int(z.shape[0])
    depths = valid = None
    if two_pass:
        if getattr(run, "depths", None) is None:
            raise ValueError("nerf_train: depth_loss_weight > 0 needs the views' depth and its standard deviation")
        depths, valid = f32(run.depths), torch.as_tensor(run.valid_depths).to(dev)
    N_rand = int(args.N_rand)
    if not 1 <= N_rand <= H * W:
        raise ValueError(f"nerf_train: N_rand {N_rand} with {H} x {W} pixels")
    perturb, noise_std = float(args.perturb) > 0., float(args.raw_noise_std)

    def draw(step, name, shape, make):
        x = rand(step, name, shape) if rand is not None else None
        return make() if x is None else x

    def uniform(step, name, shape):
        return f32(draw(step, name, shape, lambda: torch.rand(shape, generator=gen, device=dev)))

    log, last = [], start
    for i in range(start + 1, int(args.N_iters)):
        for group in optimizer.param_groups:
            group["lr"] = learning_rate(i, args.lrate, args.start_decay_lrate, args.end_decay_lrate)
        img_i = int(draw(i, "image", (), lambda: np.random.choice(n_views)))
        pix = np.asarray(draw(i, "pix", (N_rand,), lambda: np.random.choice(H * W, N_rand, replace=False)))
        pix = torch.from_numpy(pix.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
        b = ops.nerf_train_batch(intrinsics[img_i], poses[img_i], H, W, pix, images[img_i],
                                 depths[img_i] if two_pass else None, valid[img_i] if two_pass else None,
                                 z if perturb else None, uniform(i, "t_rand", (N_rand, S1)) if perturb else None)
        z1 = b["z1"] if perturb else z
        S2 = S1 if two_pass else 0
        noise = None
        if noise_std > 0.:
            noise = f32(draw(i, "noise", (N_rand, S1 + S2), lambda: torch.randn((N_rand, S1 + S2), generator=gen, device=dev))) * noise_std
        cam = embedcam.weight[img_i].detach() if embedcam is not None else None
        out = render_rays_train(model, b["rays"][:, :3], b["rays"][:, 3:], b["viewdirs"], z1, "draw" if two_pass else None, cam, bb_center,
                                bb_scale, noise, depth_range=b.get("depth_range"), u=uniform(i, "u", (N_rand, S1)) if two_pass and perturb
                                else None, lower_bound=lower_bound, near=near, far=far)
        optimizer.zero_grad()
        loss, img_loss, _ = training_loss(out, b["target_s"], b.get("target_d"), b.get("target_vd"), args.depth_loss_weight)
        loss.backward()
        torch.nn.utils.clip_grad_value_(params, 0.1)
        optimizer.step()
        last = i
        if i % args.i_weights == 0 or i + 1 == int(args.N_iters):
            name = "{:06d}.tar".format(i)
            save_checkpoint(os.path.join(run_dir, name), i, model, optimizer, embedcam)
            if not read_by_the_tools(name):
                warnings.warn(f"nerf_train: {name} is resumed from by nerf_train only: nerf_render, nerf_test and nerf_extract read the "
                              f"newest checkpoint whose name contains 000.tar (a step count that is a multiple of 1000)")
        if i % args.i_print == 0:
            mse, total = img_loss.item(), loss.item()
            psnr = -10. * float(np.log10(mse)) if mse > 0. else float("inf")
            log.append((i, total, mse, psnr))
            print(f"[TRAIN] Iter: {i} Loss: {mse}  PSNR: {psnr}")
    return SimpleNamespace(model=model, optimizer=optimizer, embedcam=embedcam, step=last, log=log)
