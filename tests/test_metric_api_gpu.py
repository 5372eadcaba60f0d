"""GPU: the public metric functions of srgan_amd.evaluation -- ``compute_frechet_distance`` and ``compute_kid`` against the float64
references and bounds of tests/metric_common.py on numpy and on device-tensor inputs, their argument errors, and
``GAN_evaluation.get_metrics`` / ``get_fd`` / ``get_kid`` on a narrow VGG19-bn (one extraction per set)."""
import numpy as np
import pytest
import torch

from tests import metric_common as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["65x63x130 shifted scaled", "130x33x257 relu swapped", "128x128x256 self"])
def test_compute_frechet_distance(name):
    from srgan_amd.evaluation import compute_frechet_distance
    x, y, ref = mc.fd_case(name)
    tol = mc.FD_TOL * ref["scale"]
    terms = compute_frechet_distance(x, y, return_terms=True)
    assert set(terms) == {"fd", "mean_term", "trace_real", "trace_fake", "nuclear", "sweeps"}
    print(f"metric fd api | {name} | sweeps {terms['sweeps']} | err / tol {abs(terms['fd'] - ref['fd']) / tol:.3f}")
    assert 1 <= terms["sweeps"] <= mc.FD_MAX_SWEEPS
    assert abs(terms["fd"] - ref["fd"]) <= tol
    assert abs(2 * (terms["nuclear"] - ref["nuclear"])) <= tol
    diff = np.abs(x.astype(np.float64).mean(axis=0) - y.astype(np.float64).mean(axis=0))
    bm = mc.mean_bound(x) + mc.mean_bound(y)
    assert abs(terms["mean_term"] - ref["mean_term"]) <= (2 * diff * bm + bm * bm).sum() + 1e-15 * ref["mean_term"]
    assert abs(terms["trace_real"] - ref["trace_real"]) <= mc.trace_bound(x)
    assert abs(terms["trace_fake"] - ref["trace_fake"]) <= mc.trace_bound(y)
    assert terms["fd"] == terms["mean_term"] + terms["trace_real"] + terms["trace_fake"] - 2.0 * terms["nuclear"]
    # device tensors give the same number bit for bit, and a plain call returns the float
    fd = compute_frechet_distance(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda())
    assert isinstance(fd, float) and fd == terms["fd"]


def test_compute_frechet_distance_with_the_larger_set_above_the_limit():
    """3 x 4100: only the smaller side is limited; vectors of 4100 elements take 17 strides of the pair workgroup"""
    from srgan_amd.evaluation import compute_frechet_distance
    r = np.random.default_rng([42])
    x, y = r.standard_normal((3, 8)).astype(np.float32), (r.standard_normal((4100, 8)) * 0.7 + 0.2).astype(np.float32)
    ref = mc.fd_ref64(x, y, return_terms=True)
    for a, b in ((x, y), (y, x)):
        terms = compute_frechet_distance(a, b, return_terms=True)
        assert abs(terms["fd"] - ref["fd"]) <= mc.FD_TOL * ref["scale"], (terms, ref)
        assert abs(2 * (terms["nuclear"] - ref["nuclear"])) <= mc.FD_TOL * ref["scale"]


def test_compute_frechet_distance_errors():
    from srgan_amd.evaluation import compute_frechet_distance
    x, y, _ = mc.fd_case("64x64x96 iid")
    with pytest.raises(ValueError, match="4096"):
        compute_frechet_distance(np.zeros((4097, 4), np.float32), np.zeros((4098, 4), np.float32))
    with pytest.raises(ValueError):
        compute_frechet_distance(x[:1], y)
    with pytest.raises(ValueError):
        compute_frechet_distance(x, y[:, :5])
    with pytest.raises(RuntimeError, match="max_sweeps"):
        compute_frechet_distance(x, y, max_sweeps=2)


@pytest.mark.parametrize("n_real,n_fake,d,subsets,size", [(150, 131, 257, 7, 130), (70, 90, 16, 100, 1000), (40, 30, 4101, 3, 64)],
                         ids=str)
def test_compute_kid(n_real, n_fake, d, subsets, size):
    from srgan_amd.evaluation import compute_kid, kid_subsets
    x, y = mc.kid_inputs(n_real, n_fake, d)
    ix, iy = kid_subsets(n_real, n_fake, subsets, size, seed=9)
    assert ix.shape == (subsets, min(n_real, n_fake, size))
    _, ref = mc.kid_ref64(x, y, ix, iy)
    _, bound = mc.kid_bound(x, y, ix, iy)
    got = compute_kid(x, y, num_subsets=subsets, max_subset_size=size, seed=9)
    assert isinstance(got, float) and abs(got - ref) <= bound, (got, ref, bound)
    assert compute_kid(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), num_subsets=subsets, max_subset_size=size, seed=9) == got


def test_kid_of_identical_distributions_is_near_zero_and_may_be_negative():
    from srgan_amd.evaluation import compute_kid
    r = np.random.default_rng([41])
    for k in range(4):
        x, y = r.standard_normal((200, 32)).astype(np.float32), r.standard_normal((200, 32)).astype(np.float32)
        v = compute_kid(x, y, num_subsets=10, max_subset_size=100, seed=k)
        assert abs(v) < 0.05
    shifted = compute_kid(x, y + np.float32(1.0), num_subsets=10, max_subset_size=100, seed=0)
    assert shifted > 0.5


def test_gan_evaluation_get_metrics():
    """GAN_evaluation("vgg-initialization") with a VGG19-bn of 1/16 width swapped in, 12 + 10 random 3 x 64 x 64 images"""
    from srgan_amd import evaluation as he
    torch.manual_seed(3)
    ev = he.GAN_evaluation("vgg-initialization", "cuda")
    ev.model = he.vgg_model(he.VGG19_bn(width_div=16).cuda().eval())
    g = torch.Generator().manual_seed(7)
    true = torch.rand(12, 3, 64, 64, generator=g) * 2 - 1
    pred = torch.rand(10, 3, 64, 64, generator=g) * 1.6 - 1
    calls = []
    feature = ev.model.model.feature
    ev.model.model.feature = lambda x: (calls.append(int(x.shape[0])), feature(x))[1]

    out = ev.get_metrics(true, pred, num_subsets=5, max_subset_size=8, seed=2)
    assert calls == [12, 10]                                     # one extraction (one batch) per set
    assert set(out) == {"precision", "recall", "density", "coverage", "fd", "kid"}
    assert out == {**out, **ev.get_prdc(true, pred)}
    f1, f2 = ev.get_feature(ev.preprocess(true)), ev.get_feature(ev.preprocess(pred))
    assert f1.shape == (12, 256) and f2.shape == (10, 256)
    assert out["fd"] == he.compute_frechet_distance(f1, f2) == ev.get_fd(true, pred)
    assert out["kid"] == he.compute_kid(f1, f2, num_subsets=5, max_subset_size=8, seed=2)
    assert out["kid"] == ev.get_kid(true, pred, num_subsets=5, max_subset_size=8, seed=2)
    ref = mc.fd_ref64(f1, f2, return_terms=True)
    assert abs(out["fd"] - ref["fd"]) <= mc.FD_TOL * ref["scale"]
    only = ev.get_metrics(true, pred, metrics=("kid",), num_subsets=5, max_subset_size=8, seed=2)
    assert only == {"kid": out["kid"]}
    with pytest.raises(ValueError, match="unknown"):
        ev.get_metrics(true, pred, metrics=("fid",))
