"""The checker of the camera-embedding optimisation (tests/nerf_camopt_ref.py) against what the reference recorded
(tests/golden/nerf_camopt.npz), and the host-only loop (nerf_rpn_amd/camopt.py) against the reference's own
optimize_camera_embedding.  No GPU.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import nerf_camopt_ref as C
from nerf_camopt_ref import camopt_bounds, camopt_golden, camopt_refs  # noqa: F401  (fixtures)
from nerf_rpn_amd import camopt
from nerf_rpn_amd.scripts import nerf_test as X
from nerf_rpn_amd.scripts import nerf_test_opt as XO

U64 = 2.0 ** -53
ALL = [(n, cam, part) for n in C.CASE_NAMES for cam in C.CAMS for part in C.PARTITIONS]


@pytest.fixture(scope="module")
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)         # the golden file was recorded with one thread
    yield
    torch.set_num_threads(threads)


def grad_bound(bounds, name, cam, part, mode="given_z2"):
    b = bounds["cases"][name]
    return b[mode]["grad"]["bound"] + np.array(b["allow"][mode][cam][part]["allow"])


@pytest.mark.parametrize("name,cam,part", ALL)
def test_float32_checker_reproduces_the_reference(camopt_refs, camopt_golden, camopt_bounds, name, cam, part):
    r = camopt_refs(name, cam, part)
    tol = camopt_bounds["golden_difference"]
    for key, got in (("losses", r["o32"]["losses"].numpy()), ("grad", r["o32"]["grad"].numpy())):
        want = camopt_golden[f"{name}/{cam}/{part}/{key}"]
        diff = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name}/{cam}/{part}/{key}: |checker - reference| {diff:.3g}, recorded largest {tol[key]:.3g}")
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want) if tol[key] == 0. else diff <= tol[key]


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_weights_and_samples_do_not_depend_on_the_embedding(camopt_refs, name):
    r = camopt_refs(name, "far", "remainder")
    c, target, rw = r["c"], r["target"], r["rw"]
    t = {cam: C.head_terms(c, C.CAMS[cam], torch.float64, r["z2"]) for cam in C.CAMS}
    for k in ("weights", "z_vals", "sigma"):
        assert torch.equal(t["zero"][k], t["far"][k]), k
    assert not torch.equal(t["zero"]["pre"], t["far"]["pre"])
    # the gradient through the reference's whole graph is the gradient with samples and weights held fixed
    fg = C.fixed_gradient(c, t["far"], target, rw)
    full = r["o64"]["grad"]
    diff, tol = (fg["grad"] - full).abs(), 16 * U64 * fg["abs_terms"]
    print(f"{name}: |full graph - fixed weights| {diff.max():.3g} at |grad| {full.abs().max():.3g}, tolerance {tol.min():.3g}")
    assert (diff <= tol).all()
    assert abs(float(fg["loss"] - r["o64"]["losses"].sum())) <= 16 * U64 * float(r["o64"]["losses"].sum())


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_gradient_against_central_differences(camopt_refs, name):
    r = camopt_refs(name, "far", "equal")
    c, h = r["c"], 1e-5
    cam = torch.tensor(C.CAMS["far"], dtype=torch.float64)
    fd = torch.zeros(4, dtype=torch.float64)
    for k in range(4):
        step = torch.zeros(4, dtype=torch.float64)
        step[k] = h
        lp = C.objective(c, cam, r["target"], r["batches"], torch.float64, r["z2"], offset=step)["losses"].sum()
        lm = C.objective(c, cam, r["target"], r["batches"], torch.float64, r["z2"], offset=-step)["losses"].sum()
        fd[k] = (lp - lm) / (2 * h)
    grad = r["o64"]["grad"]
    diff = float((fd - grad).abs().max())
    print(f"{name}: |central difference - grad| {diff:.3g} at |grad| {grad.abs().max():.3g}")
    assert diff <= 1e-3 * float(grad.abs().max())


@pytest.fixture(scope="module")
def loop_runs(camopt_golden, one_thread):
    """case -> (recorded partition, memoised float32 value_and_grad, loop result): evaluations are shared between the loop variants."""
    cache = {}

    def get(name):
        if name not in cache:
            c = C.case(name)
            sizes = camopt_golden[f"{name}/loop/sizes"].tolist()
            batches = list(torch.split(torch.from_numpy(camopt_golden[f"{name}/loop/partition"]), sizes))
            inner, memo = C.value_and_grad(c, C.target_for(c), batches, torch.float32), {}

            def f(cam):
                key = cam.numpy().tobytes()
                if key not in memo:
                    memo[key] = inner(cam)
                return memo[key]
            cache[name] = (batches, f, camopt.optimize_embedding(f, 4))
        return cache[name]
    return get


@pytest.mark.parametrize("name", C.LOOP_CASES)
def test_loop_returns_the_reference_embedding(loop_runs, camopt_golden, name):
    batches, _, got = loop_runs(name)
    want = camopt_golden[f"{name}/loop/embedding"]
    print(f"{name}: loop {got.tolist()}, reference {want.tolist()}, batches {[len(b) for b in batches]}")
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert len(set(len(b) for b in batches)) == 2          # the recorded partition has a remainder batch


def test_loop_returns_zero_if_no_psnr_beats_zero():
    calls = []

    def f(cam):
        calls.append(cam.clone())
        return 4.0, torch.ones(3)             # PSNR -6 dB at every step
    assert torch.equal(camopt.optimize_embedding(f, 3, steps=5), torch.zeros(3)) and len(calls) == 5
    assert torch.equal(calls[0], torch.zeros(3)) and calls[0].dtype == torch.float32 and not torch.equal(calls[1], calls[0])


@pytest.mark.parametrize("quirk", ["min_mode", "best_before_step", "last"])
def test_loop_mutations_miss_the_reference(loop_runs, camopt_golden, quirk):
    """The unmutated loop equals the recorded embedding bit for bit, so the unit is the embedding's float32 spacing: more than 10 of
    them off in some case."""
    worst = 0.
    for name in C.LOOP_CASES:
        _, f, _ = loop_runs(name)
        got, want = camopt.optimize_embedding(f, 4, quirk=quirk), camopt_golden[f"{name}/loop/embedding"]
        ulps = float(np.abs(got.numpy() - want).max()) / (2.0 ** -23 * float(np.abs(want).max()))
        print(f"{quirk}, {name}: embedding differs from the reference's by {ulps:.3g} float32 spacings")
        worst = max(worst, ulps)
    assert worst > 10


def test_random_subsets_and_ray_weights():
    parts = camopt.random_subsets(15, 4, torch.Generator().manual_seed(5))
    assert [len(p) for p in parts] == [4, 4, 4, 3] and sorted(torch.cat(parts).tolist()) == list(range(15))
    assert torch.equal(torch.cat(parts), torch.randperm(15, generator=torch.Generator().manual_seed(5)))
    rw = camopt.ray_weights(parts, 15)
    assert rw.dtype == torch.float64 and torch.equal(rw, C.ray_weights(parts, 15))
    assert float(rw[parts[0][0]]) == 1. / 12. and float(rw[parts[3][0]]) == 1. / 9.
    with pytest.raises(ValueError):
        camopt.ray_weights(parts[:3], 15)
    # H W a multiple of the subset size: every ray weighs 1 / (3 subset), whatever the permutation
    a, b = (camopt.ray_weights(camopt.random_subsets(16, 4, torch.Generator().manual_seed(s)), 16) for s in (1, 2))
    assert torch.equal(a, b) and torch.equal(a, torch.full((16,), 1. / 12., dtype=torch.float64))


def test_partition_matters_only_with_a_remainder_batch(camopt_refs, camopt_bounds):
    name = "odd_5x7"
    r = camopt_refs(name, "far", "equal")
    c, n = r["c"], C.num_rays(r["c"])
    other = C.partition(n, "equal", seed=1)
    assert not torch.equal(torch.cat(other), torch.cat(r["batches"]))
    o = C.objective(c, C.CAMS["far"], r["target"], other, torch.float32)
    m0, m1 = float(r["o32"]["m"]), float(o["m"])
    print(f"equal batches, two partitions: m {m0!r} and {m1!r}")
    assert abs(m0 - m1) <= 2 * len(other) * 2.0 ** -24 * m0            # the float32 batch sums, nothing else
    assert torch.equal(C.ray_weights(other, n), r["rw"])
    # with a remainder batch the rays do not weigh the same: a uniform weight gives another gradient
    rr = camopt_refs(name, "far", "remainder")
    t = C.head_terms(c, C.CAMS["far"], torch.float64, rr["z2"])
    good = C.fixed_gradient(c, t, rr["target"], rr["rw"])["grad"]
    flat = C.fixed_gradient(c, t, rr["target"], C.ray_weights(rr["batches"], n, uniform=True))["grad"]
    diff, bound = (good - flat).abs().numpy(), grad_bound(camopt_bounds, name, "far", "remainder")
    print(f"uniform ray weights with a remainder batch: gradient off by {diff.max():.3g}, bound {bound.max():.3g}")
    assert (diff > 10 * bound).any()


@pytest.mark.parametrize("mutation", C.GRAD_MUTATIONS)
def test_gradient_mutations_exceed_the_bound(camopt_refs, camopt_bounds, mutation):
    name = "views_cam_3x5"
    r = camopt_refs(name, "far", "remainder")
    t = C.head_terms(r["c"], C.CAMS["far"], torch.float64, r["z2"])
    got = C.fixed_gradient(r["c"], t, r["target"], r["rw"], mutation)["grad"]
    diff, bound = (got - r["o64"]["grad"]).abs().numpy(), grad_bound(camopt_bounds, name, "far", "remainder")
    print(f"{mutation}: gradient off by {diff.max():.3g}, bound {bound.max():.3g}")
    assert (diff > 10 * bound).any()


def test_parser_flags_and_directories():
    p = XO.build_parser()
    base = ["--expname", "e", "--ckpt_dir", "c", "--scene_id", "s"]
    a = p.parse_args(base)
    assert XO.result_dir(a) == os.path.join("c", "e", "test_images_with_optimization_s")
    assert XO.latent_code_dir(a) == os.path.join("c", "e", "test_latent_codes_s")
    assert XO.TRANSFORMS == X.TASKS["test"][0] == "transforms_test.json"
    assert (a.N_rand, a.opt_steps, a.opt_seed, a.opt_cache_gib, a.output_dir) == (None, 100, 0, None, None)
    b = p.parse_args(base + ["--N_rand", "8", "--opt_steps", "4", "--opt_seed", "3", "--opt_cache_gib", "0.5", "--output_dir", "o"])
    assert (b.N_rand, b.opt_steps, b.opt_seed, b.opt_cache_gib) == (8, 4, 3, 0.5) and XO.result_dir(b) == "o"
    with pytest.raises(SystemExit, match="nerf_test_opt: --expname"):
        XO.main([])
    # nerf_test keeps its tasks and directories
    t = X.build_parser()
    assert sorted(X.TASKS) == ["render_train_depth", "test"]
    assert X.result_dir(t.parse_args(base)) == os.path.join("c", "e", "test_images_s")
    assert X.result_dir(t.parse_args(base + ["--task", "render_train_depth"])) == os.path.join("c", "e", "train_depth_s")
    assert X.TASKS["test"] == ("transforms_test.json", "test_images_") and X.TASKS["render_train_depth"] == ("transforms_train.json", "train_depth_")
