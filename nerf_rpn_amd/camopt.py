"""The loop of the test-time optimisation of the camera embedding (reference data/scannet/run_nerf.py, optimize_camera_embedding
:193-229), host-only: the objective is a callable, so the loop runs on the CPU against any implementation of it
(ops.nerf_camopt_eval in scripts/nerf_test_opt.py, the torch checker in the tests).

What the reference does, quirks included: the embedding starts at zero; Adam(lr=0.5) and ReduceLROnPlateau('max', factor=0.5,
patience=3) on the PSNR; per step the gradients of the per-batch mean squared errors are summed over the batches (:212-221), the
optimizer steps (:222), the PSNR of the mean m of the batch losses *before* that step is handed to the scheduler (:223-224), and if it
beats the best so far (initially 0) the embedding *after* the step is kept (:225-227).  The kept embedding is returned; if no PSNR
ever exceeds 0 that is the zero vector.

Assumption: create_random_subsets lives in the Dense-Depth-Priors code, which is not part of the reference; it is taken
to split a torch.randperm of the indices into consecutive pieces of the subset size, the remainder being the last piece.
"""
import torch

LR, FACTOR, PATIENCE = 0.5, 0.5, 3


def random_subsets(n, subset_size, generator=None):
    """The assumed create_random_subsets(range(n), subset_size): a random permutation of 0 .. n - 1 cut into consecutive pieces of
    subset_size, the remainder as the last piece -> list of int64 tensors."""
    perm = torch.randperm(int(n), generator=generator)
    return list(torch.split(perm, int(subset_size)))


def ray_weights(batches, n):
    """The weight of each ray's squared error in the sum of the batch means (:219-221): 1 / (3 n_b) for a ray in a batch of n_b rays
    -> float64 [n].  The batches must partition 0 .. n - 1."""
    rw = torch.zeros(int(n), dtype=torch.float64)
    seen = torch.zeros(int(n), dtype=torch.int64)
    for b in batches:
        rw[b] = 1. / (3. * len(b))
        seen[b] += 1
    if not bool((seen == 1).all()):
        raise ValueError("the batches do not partition the rays")
    return rw


def mse2psnr(m):
    """The fork's mse2psnr in the dtype of m (a tensor, or a Python float taken as float64)."""
    m = m if isinstance(m, torch.Tensor) else torch.tensor(float(m), dtype=torch.float64)
    return -10. * torch.log(m) / torch.log(torch.full((1,), 10., dtype=m.dtype))


def optimize_embedding(value_and_grad, cam_ch, steps=100, quirk=None):
    """value_and_grad(cam) -> (m, grad): the mean over the batches of the batch MSE at the float32 embedding ``cam`` [cam_ch] (a
    number or a tensor; the PSNR is computed in its dtype) and its gradient [cam_ch].  -> the best embedding, float32 [cam_ch].
    ``quirk`` (tests only) breaks one property of the loop: "min_mode", "best_before_step" or "last"."""
    assert quirk in (None, "min_mode", "best_before_step", "last")
    cam = torch.zeros(int(cam_ch), dtype=torch.float32, requires_grad=True)
    optimizer = torch.optim.Adam(params=(cam,), lr=LR)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, 'min' if quirk == "min_mode" else 'max', factor=FACTOR,
                                                           patience=PATIENCE)
    max_psnr = 0
    best = torch.zeros(int(cam_ch), dtype=torch.float32)
    for _ in range(int(steps)):
        optimizer.zero_grad()
        m, grad = value_and_grad(cam.detach().clone())
        cam.grad = torch.as_tensor(grad).detach().to(device="cpu", dtype=torch.float32).reshape(cam.shape).clone()
        before = cam.detach().clone()
        optimizer.step()
        psnr = mse2psnr(m).reshape(-1)[0]
        scheduler.step(psnr)
        if psnr > max_psnr or quirk == "last":
            max_psnr = psnr
            best = before if quirk == "best_before_step" else cam.detach().clone()
    return best
