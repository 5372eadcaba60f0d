"""Evaluation path of the reference (``pyfiles/evaluation.py``) on the MI355X kernels.

Same names and call signatures as the reference module: ``vgg_model`` (evaluation.py:13-36), ``GAN_evaluation`` with
``preprocess`` / ``get_feature`` / ``get_prdc`` (:38-110), ``evaluation_init`` (:112-122).  Two third-party pieces the reference
imports are not in this image and are provided here:

* ``VGG19_bn`` -- torchvision's ``models.vgg19_bn`` as a parameter holder with torchvision's ``state_dict`` keys, shapes and
  default initialisation, so the reference's ``.pth`` files (ImageNet / the CelebA facial recogniser) load unchanged.  In
  eval mode every BatchNorm is folded into its convolution once (``fold()``); the forward is 16 fused conv + bias + ReLU
  launches on the train step's Winograd / implicit-GEMM kernels, five 2x2 max pools and the two Linear layers as 1x1
  convolutions (flattened in NCHW order like ``torch.flatten``).  Inference only (no backward).
* ``compute_prdc`` -- prdc 0.2's function of that name over the HIP distance / k-th value / set-statistics kernels.

Beyond the reference (csrc/metrics.hip): ``compute_frechet_distance`` (FID's formula over whatever features it is
given), ``compute_kid`` / ``kid_subsets`` (Kernel Inception Distance, StyleGAN2-ADA's estimator) and the ``get_fd`` /
``get_kid`` / ``get_metrics`` methods of ``GAN_evaluation``.  Over the VGG19-bn features of this path the Frechet number is NOT
comparable with published Inception-v3 FIDs; it ranks runs of this project against each other.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .inference import cuda2numpy, image_from_output
from .losses import weights_init
from .ops import ACT_NONE, ACT_RELU, PAD_ZERO

__all__ = ["VGG19_bn", "vgg19_bn", "vgg_model", "GAN_evaluation", "evaluation_init", "compute_prdc", "maxpool2",
           "compute_frechet_distance", "compute_kid", "kid_subsets", "FD_MAX_SIDE", "compute_style_diversity", "compute_ssim",
           "compute_psnr"]

VGG19_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


def maxpool2(x):
    """nn.MaxPool2d(2, 2) on an NHWC-dense activation (inference)."""
    x = ops.to_nhwc(x)
    n, c, h, w = x.shape
    y = ops.nhwc_empty(n, c, h // 2, w // 2, x.device)
    _lib.check(_lib.load().srgan_maxpool2_fwd(ops._ptr(x), ops._ptr(y), n, h, w, c, ops._stream()), "maxpool2_fwd")
    return y


class _MaxPool(nn.Module):
    def forward(self, x):
        return maxpool2(x)


class _Holder(nn.Module):
    """Parameter-free slot (ReLU / Dropout / AdaptiveAvgPool2d) that keeps torchvision's Sequential indices."""

    def forward(self, x):
        return x


class VGG19_bn(nn.Module):
    def __init__(self, num_classes=1000, width_div=1):
        super().__init__()
        layers, cin = [], 3
        for v in VGG19_CFG:
            if v == "M":
                layers.append(_MaxPool())
                continue
            c = v // width_div
            layers += [nn.Conv2d(cin, c, kernel_size=3, padding=1), nn.BatchNorm2d(c), _Holder()]
            cin = c
        self.features = nn.Sequential(*layers)
        self.avgpool = _Holder()                   # AdaptiveAvgPool2d((7, 7)): the identity on the 224x224 inputs of the path
        hid = 4096 // width_div
        self.classifier = nn.Sequential(nn.Linear(cin * 49, hid), _Holder(), _Holder(), nn.Linear(hid, hid), _Holder(), _Holder(),
                                        nn.Linear(hid, num_classes))
        for m in self.modules():                   # torchvision.models.vgg.VGG._initialize_weights
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)
        self._folded = None

    def fold(self):
        """Eval-mode BatchNorm folded into the preceding convolution: w' = w * g / sqrt(var + eps), b' = (b - mean) * g /
        sqrt(var + eps) + beta.  One-time parameter preparation (re-run after loading weights)."""
        folded, mods = [], list(self.features)
        with torch.no_grad():
            for i, m in enumerate(mods):
                if isinstance(m, nn.Conv2d):
                    bn = mods[i + 1]
                    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
                    folded.append(((m.weight * s.view(-1, 1, 1, 1)).contiguous(), ((m.bias - bn.running_mean) * s + bn.bias).contiguous()))
                elif isinstance(m, _MaxPool):
                    folded.append(None)
        self._folded = folded
        return self

    def load_state_dict(self, *a, **k):
        self._folded = None
        return super().load_state_dict(*a, **k)

    def _features(self, x):
        if self.training:
            raise NotImplementedError("VGG19_bn runs in eval mode only (the evaluation path never trains it): call .eval()")
        if self._folded is None or self._folded[0][0].device != x.device:
            self.fold()
        x = ops.to_nhwc(x)
        for f in self._folded:
            x = maxpool2(x) if f is None else ops.conv2d(x, f[0], f[1], 1, 1, PAD_ZERO, ACT_RELU)
        n, c, h, w = x.shape
        if (h, w) != (7, 7):
            raise NotImplementedError(f"VGG19_bn: expected 224x224 inputs (7x7 final map), got a {h}x{w} final map")
        return ops.to_nchw(x).reshape(n, c * h * w, 1, 1)          # torch.flatten(x, 1) order

    @staticmethod
    def _linear(x, lin, act):
        return ops.conv2d(x, lin.weight.view(lin.out_features, lin.in_features, 1, 1), lin.bias, 1, 0, PAD_ZERO, act)

    def feature(self, x):
        """features -> avgpool -> flatten -> classifier[:6]  ([N, 4096])."""
        with torch.no_grad(), ops.pack_cache():
            h = self._features(x)
            h = self._linear(h, self.classifier[0], ACT_RELU)
            h = self._linear(h, self.classifier[3], ACT_RELU)
            return h.reshape(h.shape[0], -1)

    def forward(self, x):
        with torch.no_grad(), ops.pack_cache():
            h = self.feature(x)
            h = self._linear(h.reshape(h.shape[0], -1, 1, 1), self.classifier[6], ACT_NONE)
            return h.reshape(h.shape[0], -1)


def vgg19_bn(pretrained=False, **kw):
    """``torchvision.models.vgg19_bn``.  ``pretrained=True`` needs torchvision's weight file, which this image does not have:
    load it yourself with ``load_state_dict`` (the keys are torchvision's)."""
    if pretrained:
        raise NotImplementedError("vgg19_bn(pretrained=True): no network / torchvision here -- build the model and "
                                  "load_state_dict() the ImageNet weights from a file")
    return VGG19_bn(**kw)


class vgg_model():
    """evaluation.py:13-36: ``get(x, "feature")`` = classifier[:6] output, ``get(x, "score")`` = the full model."""

    def __init__(self, model):
        self.model = model

    def get(self, x, output_type="score"):
        if output_type == "feature":
            return self.model.feature(x)
        elif output_type == "score":
            return self.model(x)


def _dev_f32(a, device):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32) if not torch.is_tensor(a) else a.to(torch.float32)
    return t.to(device).contiguous()


def compute_prdc(real_features, fake_features, nearest_k, device="cuda"):
    """prdc.compute_prdc(real_features, fake_features, nearest_k) -> dict(precision, recall, density, coverage).
    ``nearest_k`` <= 15 (the reference's notebooks use 5, evaluation.py:85-110): the k-th-neighbour kernel keeps its candidates
    in registers (``KTH_MAX`` = 16 slots per lane, csrc/evaluation.hip); a larger k raises ``ValueError`` here instead of a C-ABI
    error from inside the launch sequence."""
    if not 1 <= int(nearest_k) <= 15:
        raise ValueError(f"compute_prdc: nearest_k = {nearest_k} outside 1..15 (register-resident k-th-neighbour kernel)")
    lib = _lib.load()
    x, y = _dev_f32(real_features, device), _dev_f32(fake_features, device)
    n, d = x.shape
    m = y.shape[0]
    if y.shape[1] != d:
        raise ValueError("compute_prdc: feature dimensions differ")
    st = ops._stream()

    def dist(a, b):
        out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
        _lib.check(lib.srgan_pairwise_dist(ops._ptr(a), a.shape[0], ops._ptr(b), b.shape[0], d, ops._ptr(out), st), "pairwise_dist")
        return out

    def radii(a):
        dm = dist(a, a)
        out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
        _lib.check(lib.srgan_kth_smallest_rows(ops._ptr(dm), a.shape[0], a.shape[0], nearest_k + 1, ops._ptr(out), st), "kth_smallest_rows")
        return out

    r_real, r_fake = radii(x), radii(y)
    drf = dist(x, y)
    out4 = torch.empty(4, dtype=torch.float32, device=x.device)
    nb = lib.srgan_prdc_workspace(n, m)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    _lib.check(lib.srgan_prdc_from_dist(ops._ptr(drf), n, m, ops._ptr(r_real), ops._ptr(r_fake), int(nearest_k), ops._ptr(out4),
                                        ops._ptr(ws), nb, st), "prdc_from_dist")
    p, r, dn, c = (float(v) for v in out4.cpu())
    return dict(precision=p, recall=r, density=dn, coverage=c)


FD_MAX_SIDE = 4096        # the smaller set of compute_frechet_distance: its Gram matrix W [n, L] is what the Jacobi sweeps work on


def _feature_pair(real_features, fake_features, who):
    """Shape checks on the host arrays / tensors as given (before anything touches the library)."""
    rs, fs = tuple(real_features.shape), tuple(fake_features.shape)
    if len(rs) != 2 or len(fs) != 2:
        raise ValueError(f"{who}: features must be [N, D] matrices, got {rs} and {fs}")
    if rs[1] != fs[1]:
        raise ValueError(f"{who}: feature dimensions differ ({rs[1]} and {fs[1]})")
    if rs[1] < 1:
        raise ValueError(f"{who}: no feature columns")
    return rs[0], fs[0], rs[1]


def _feature_stats(lib, x, st):
    """(mean [D] fp32, A = (x - mean) / sqrt(N - 1) fp32, trace: 1-element float64 tensor) on the device."""
    n, d = x.shape
    mean = torch.empty(d, dtype=torch.float32, device=x.device)
    a = torch.empty_like(x)
    trace = torch.empty(1, dtype=torch.float64, device=x.device)
    nb = lib.srgan_feature_stats_workspace(n, d)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
    _lib.check(lib.srgan_feature_stats(ops._ptr(x), n, d, ops._ptr(mean), ops._ptr(a), ops._ptr(trace), ops._ptr(ws), nb, st),
               "feature_stats")
    return mean, a, trace


def compute_frechet_distance(real_features, fake_features, device="cuda", max_sweeps=30, return_terms=False):
    """pytorch-fid's ``calculate_frechet_distance`` on the sets' means and unbiased covariances (``np.cov``):
    ``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)``, a Python float, not clamped at 0.  ``tr sqrt(S1 S2)`` is the nuclear
    norm of ``A1 A2^T`` with ``A = (X - mean) / sqrt(N - 1)``: only that ``n1 x n2`` matrix is decomposed (one-sided Jacobi sweeps
    over its shorter side until a sweep rotates nothing; the host reads one counter per sweep).  ``return_terms=True``: a dict of
    ``fd``, the four terms (``mean_term``, ``trace_real``, ``trace_fake``, ``nuclear``) and ``sweeps``."""
    n1, n2, d = _feature_pair(real_features, fake_features, "compute_frechet_distance")
    if n1 < 2 or n2 < 2:
        raise ValueError(f"compute_frechet_distance: a set has fewer than 2 rows ({n1} and {n2}): no covariance")
    if min(n1, n2) > FD_MAX_SIDE:
        raise ValueError(f"compute_frechet_distance: the smaller set has {min(n1, n2)} rows, the limit is {FD_MAX_SIDE}")
    if int(max_sweeps) < 1:
        raise ValueError("compute_frechet_distance: max_sweeps must be at least 1")
    lib = _lib.load()
    x, y = _dev_f32(real_features, device), _dev_f32(fake_features, device)
    st = ops._stream()
    mu1, a1, t1 = _feature_stats(lib, x, st)
    mu2, a2, t2 = _feature_stats(lib, y, st)
    # the shorter side carries the vectors: n = min(n1, n2) of length L = max(n1, n2)
    p, q = (a1, a2) if n1 <= n2 else (a2, a1)
    n, length = p.shape[0], q.shape[0]
    w = torch.empty(n, length, dtype=torch.float32, device=x.device)
    _lib.check(lib.srgan_gram_f32(ops._ptr(p), n, None, n, ops._ptr(q), length, None, length, d, ops._ptr(w), st), "gram_f32")
    nb = lib.srgan_jacobi_workspace(n)
    ws = torch.empty(-(-nb // 8), dtype=torch.float64, device=x.device)
    count = torch.empty(1, dtype=torch.int32, device=x.device)
    sweeps = 0
    while True:
        if sweeps == int(max_sweeps):
            raise RuntimeError(f"compute_frechet_distance: the Jacobi sweeps still rotated after max_sweeps = {max_sweeps}")
        _lib.check(lib.srgan_jacobi_sweep(ops._ptr(w), n, length, ops._ptr(count), ops._ptr(ws), nb, st), "jacobi_sweep")
        sweeps += 1
        if int(count.item()) == 0:
            break
    nuc = torch.empty(1, dtype=torch.float64, device=x.device)
    _lib.check(lib.srgan_nuclear_from_rows(ops._ptr(w), n, length, ops._ptr(nuc), ops._ptr(ws), nb, st), "nuclear_from_rows")
    diff = mu1.cpu().numpy().astype(np.float64) - mu2.cpu().numpy().astype(np.float64)
    mean_term = float(np.dot(diff, diff))
    tr1, tr2, nuclear = float(t1.item()), float(t2.item()), float(nuc.item())
    fd = mean_term + tr1 + tr2 - 2.0 * nuclear
    if return_terms:
        return dict(fd=fd, mean_term=mean_term, trace_real=tr1, trace_fake=tr2, nuclear=nuclear, sweeps=sweeps)
    return fd


def kid_subsets(n_real, n_fake, num_subsets, max_subset_size, seed):
    """The subset tables of ``compute_kid``: two int32 arrays [num_subsets, m], m = min(n_real, n_fake, max_subset_size); row s
    is ``np.random.default_rng([seed, s, which]).choice(n, m, replace=False)`` (which = 0 real, 1 fake)."""
    n_real, n_fake, num_subsets, max_subset_size = int(n_real), int(n_fake), int(num_subsets), int(max_subset_size)
    if num_subsets < 1:
        raise ValueError("kid_subsets: num_subsets must be at least 1")
    m = min(n_real, n_fake, max_subset_size)
    if m < 1:
        raise ValueError("kid_subsets: an empty set or max_subset_size < 1")
    tabs = []
    for which, n in enumerate((n_real, n_fake)):
        tabs.append(np.stack([np.random.default_rng([int(seed), s, which]).choice(n, m, replace=False)
                              for s in range(num_subsets)]).astype(np.int32))
    return tabs[0], tabs[1]


def compute_kid(real_features, fake_features, num_subsets=100, max_subset_size=1000, seed=0, device="cuda"):
    """Kernel Inception Distance in StyleGAN2-ADA's ``kernel_inception_distance`` estimator with k(x, y) = (x . y / D + 1)^3:
    ``(1 / S) sum_s [(Sxx_s + Syy_s) / (m (m - 1)) - 2 Sxy_s / m^2]`` over S = ``num_subsets`` subsets of m rows
    (``kid_subsets``), Sxx / Syy the off-diagonal sums, Sxy the full sum.  Unbiased: it may be negative.  A Python float."""
    n1, n2, d = _feature_pair(real_features, fake_features, "compute_kid")
    if not 1 <= int(num_subsets) <= 65535:
        raise ValueError(f"compute_kid: num_subsets = {num_subsets} outside 1..65535")
    m = min(n1, n2, int(max_subset_size))
    if m < 2:
        raise ValueError(f"compute_kid: subset size min(n_real, n_fake, max_subset_size) = {m}, the estimator needs at least 2")
    ix, iy = kid_subsets(n1, n2, num_subsets, max_subset_size, seed)
    lib = _lib.load()
    x, y = _dev_f32(real_features, device), _dev_f32(fake_features, device)
    st = ops._stream()
    s = int(num_subsets)
    dx, dy = torch.as_tensor(ix).to(x.device), torch.as_tensor(iy).to(x.device)
    sums = torch.empty(s, 3, dtype=torch.float64, device=x.device)
    kid = torch.empty(1, dtype=torch.float64, device=x.device)
    nb = lib.srgan_kid_workspace(s, m)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=x.device)
    _lib.check(lib.srgan_kid_poly3(ops._ptr(x), n1, ops._ptr(y), n2, d, ops._ptr(dx), ops._ptr(dy), s, m, ops._ptr(sums),
                                   ops._ptr(kid), ops._ptr(ws), nb, st), "kid_poly3")
    return float(kid.item())


def compute_style_diversity(images):
    """Pixel-space style diversity of translations: ``images[S, N, ...]`` on the device, S styles of each of N sources -> the mean,
    over the N sources and the S (S - 1) / 2 style pairs, of ``mean |a - b|`` (``ops.rowwise_l1``: one launch per style pair over
    the N rows; the mean over the N S (S - 1) / 2 float64 row values is their exactly rounded sum, ``math.fsum``, over their number).  The number mode-seeking regularisation
    (``srgan_amd.diversity``) is meant to raise.  A Python float."""
    if not torch.is_tensor(images) or images.dim() < 3:
        raise ValueError("compute_style_diversity: a tensor [S, N, ...] expected (S styles of N sources)")
    s, n = int(images.shape[0]), int(images.shape[1])
    if s < 2:
        raise ValueError(f"compute_style_diversity: S = {s} styles; a pair needs at least 2")
    if n < 1:
        raise ValueError("compute_style_diversity: no sources")
    flat = images.to(torch.float32).reshape(s, n, -1).contiguous()
    rows = [ops.rowwise_l1(flat[i], flat[j]) for i in range(s) for j in range(i + 1, s)]
    values = torch.cat(rows).to(torch.float64).cpu().tolist()
    return math.fsum(values) / len(values)


def _image_pair(a, b, who):
    """two image sets [N, C, H, W] of one shape as CPU or device fp32 tensors (numpy arrays or tensors go in)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dim() != 4 or a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f"{who}: two image sets [N, C, H, W] of one shape expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return a.to(torch.float32), b.to(torch.float32)


def _pair_chunks(a, b, chunk, who):
    """slices of at most ``chunk`` samples; by default as many as keep one call under 2^31 floats (the kernels' offset limit)"""
    per = int(a[0].numel())
    limit = ((1 << 31) - 1) // per
    if limit < 1:
        raise ValueError(f"{who}: one image of {per} values is past the kernels' 2^31 limit")
    if chunk is None:
        chunk = limit
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"{who}: chunk must be a positive integer, got {chunk!r}")
    chunk = min(chunk, limit)
    for i in range(0, a.shape[0], chunk):
        yield a[i:i + chunk], b[i:i + chunk]


def compute_ssim(a, b, window=11, sigma=1.5, k1=0.01, k2=0.03, data_range=2.0, device="cuda", chunk=None):
    """Per-sample structural similarity of two image sets [N, C, H, W] (C <= 3; numpy arrays or tensors, paired by index) as a
    float32 numpy array [N]: Gaussian window of ``window`` taps and ``sigma``, valid positions only, the mean over a sample's
    positions and channels (``srgan_amd.structural``; the kernels of ``csrc/ssim.hip``).  ``data_range`` 2 fits images in [-1, 1].
    The sets go through the device in slices of ``chunk`` samples (default: as many as stay under the kernels' 2^31 values)."""
    from .structural import SSIM
    a, b = _image_pair(a, b, "compute_ssim")
    metric = SSIM(1.0, window, sigma, k1, k2, data_range)
    out = [metric.value(x.to(device), y.to(device)).cpu().numpy() for x, y in _pair_chunks(a, b, chunk, "compute_ssim")]
    return np.concatenate(out)


def compute_psnr(a, b, data_range=2.0, device="cuda", chunk=None):
    """Per-sample ``10 log10(data_range^2 / mse)`` of two image sets of one shape (numpy arrays or tensors, paired by index) as a
    float64 numpy array [N]; ``inf`` where a pair is equal.  Chunked as ``compute_ssim``."""
    a, b = _image_pair(a, b, "compute_psnr")
    if not (isinstance(data_range, (int, float)) and not isinstance(data_range, bool) and 0 < data_range < float("inf")):
        raise ValueError(f"compute_psnr: data_range must be finite and > 0, got {data_range!r}")
    out = [ops.psnr(x.to(device), y.to(device), data_range).cpu().numpy() for x, y in _pair_chunks(a, b, chunk, "compute_psnr")]
    return np.concatenate(out)


class GAN_evaluation():
    """evaluation.py:38-110.  ``feature_extractor``: "vgg-initialization" (default-initialised VGG19-bn, as the reference's
    ``models.vgg19_bn(pretrained=False)`` + the no-op ``weights_init``), or "vgg-ImageNet" / "vgg-CelebA" with ``weights=`` a
    path to (or a dict of) torchvision-keyed parameters -- the reference downloads / reads them from files this image lacks."""

    def __init__(self, feature_extractor="vgg-initialization", device="cuda", classes=tuple(range(4)), reference=tuple(range(4)),
                 weights=None):
        self.fe = feature_extractor
        if "vgg" not in self.fe:
            raise NotImplementedError("GAN_evaluation: only the vgg feature extractors of the reference exist")
        if "CelebA" in self.fe:
            model = VGG19_bn(num_classes=len(classes))
        else:
            model = VGG19_bn()
        if "initialization" in self.fe:
            model.apply(weights_init)
        else:
            if weights is None:
                raise FileNotFoundError(f"GAN_evaluation({self.fe!r}): pass weights=<.pth path or state_dict> (torchvision keys); "
                                        "the reference's files are not in this image")
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, str) else weights
            model.load_state_dict(sd)
        model.eval()
        self.model = vgg_model(model.to(device))
        self.device = device

    def preprocess(self, tensor):
        """Every image: 8-bit rendering (``image_from_output``), Resize((128,128)) -> Resize((224,224)) -> ToTensor ->
        Normalize(ImageNet mean / std)   (evaluation.py:61-66, 72-81).  Host side, as in the reference (PIL)."""
        from PIL import Image
        mean = np.asarray((0.485, 0.456, 0.406), np.float32)[:, None, None]
        std = np.asarray((0.229, 0.224, 0.225), np.float32)[:, None, None]
        images = []
        for i in range(tensor.shape[0]):
            im = image_from_output(tensor[i:i + 1, :, :, :])[0]
            im = im.resize((128, 128), Image.BILINEAR).resize((224, 224), Image.BILINEAR)
            a = np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0
            images.append((a - mean) / std)
        return torch.Tensor(np.array(images))

    def get_feature(self, tensor, batch=32, get_attention=False, thres=0.5):
        num = tensor.shape[0]
        features = None
        for itr in range(num // batch + int(bool(num - batch * (num // batch)))):
            data = tensor[itr * batch:(itr + 1) * batch].to(self.device)
            feature = cuda2numpy(self.model.get(data, "feature").reshape(data.shape[0], -1))
            features = feature if features is None else np.concatenate([features, feature], axis=0)
        return features

    def get_prdc(self, true, pred, nearest_k=5, preprocess=True, thres=0.5, batch=32):
        self.run_preprocess = preprocess
        if preprocess:
            true = self.preprocess(true)
            pred = self.preprocess(pred)
        f1 = self.get_feature(true)
        f2 = self.get_feature(pred)
        if f1.shape[1] == 0:
            return {"precision": None, "recall": None, "density": None, "coverage": None}
        return compute_prdc(real_features=f1, fake_features=f2, nearest_k=nearest_k, device=self.device)

    def _features_of(self, true, pred, preprocess):
        """Each set through the extractor once."""
        self.run_preprocess = preprocess
        if preprocess:
            true = self.preprocess(true)
            pred = self.preprocess(pred)
        return self.get_feature(true), self.get_feature(pred)

    def get_fd(self, true, pred, preprocess=True):
        """Frechet distance of the two sets' features (``compute_frechet_distance``); not an Inception-v3 FID."""
        f1, f2 = self._features_of(true, pred, preprocess)
        return compute_frechet_distance(f1, f2, device=self.device)

    def get_kid(self, true, pred, num_subsets=100, max_subset_size=1000, seed=0, preprocess=True):
        f1, f2 = self._features_of(true, pred, preprocess)
        return compute_kid(f1, f2, num_subsets=num_subsets, max_subset_size=max_subset_size, seed=seed, device=self.device)

    def get_diversity(self, images):
        """Pixel-space style diversity of ``images[S, N, ...]`` (``compute_style_diversity``): no feature extraction."""
        return compute_style_diversity(torch.as_tensor(images).to(self.device))

    def get_ssim(self, true, pred, **kw):
        """Per-sample SSIM of ``pred`` against ``true``, paired by index, on the raw images (``compute_ssim``): no feature extraction."""
        return compute_ssim(true, pred, device=self.device, **kw)

    def get_psnr(self, true, pred, **kw):
        """Per-sample PSNR of ``pred`` against ``true``, paired by index, on the raw images (``compute_psnr``)."""
        return compute_psnr(true, pred, device=self.device, **kw)

    def get_metrics(self, true, pred, metrics=("prdc", "fd", "kid"), nearest_k=5, num_subsets=100, max_subset_size=1000, seed=0,
                    preprocess=True, styles=None):
        """The chosen metrics from ONE extraction of each set, as one flat dict: precision / recall / density / coverage
        ("prdc"), ``fd``, ``kid``; ``diversity`` only when asked for, from ``styles[S, N, ...]`` (``get_diversity``); ``ssim`` and
        ``psnr`` only when asked for: the means over the pairs ``(true[i], pred[i])`` of the raw images (``get_ssim``, ``get_psnr``)."""
        unknown = [m for m in metrics if m not in ("prdc", "fd", "kid", "diversity", "ssim", "psnr")]
        if unknown:
            raise ValueError(f"get_metrics: unknown metrics {unknown} (prdc, fd, kid, diversity, ssim, psnr)")
        if "diversity" in metrics and styles is None:
            raise ValueError("get_metrics: 'diversity' needs styles=[S, N, ...], S translations of each of N sources")
        out = {}
        if "ssim" in metrics:
            out["ssim"] = float(np.mean(self.get_ssim(true, pred), dtype=np.float64))
        if "psnr" in metrics:
            out["psnr"] = float(np.mean(self.get_psnr(true, pred)))
        if out and all(m in ("ssim", "psnr") for m in metrics):
            return out                         # pixel-space metrics alone: no feature extraction
        f1, f2 = self._features_of(true, pred, preprocess)
        if "prdc" in metrics:
            out.update(compute_prdc(real_features=f1, fake_features=f2, nearest_k=nearest_k, device=self.device))
        if "fd" in metrics:
            out["fd"] = compute_frechet_distance(f1, f2, device=self.device)
        if "kid" in metrics:
            out["kid"] = compute_kid(f1, f2, num_subsets=num_subsets, max_subset_size=max_subset_size, seed=seed, device=self.device)
        if "diversity" in metrics:
            out["diversity"] = self.get_diversity(styles)
        return out


def evaluation_init(fe_list, classes, metrics):
    """Nested result store fe -> source -> target -> metric -> []   (evaluation.py:112-122)."""
    return {fe: {s: {t: {m: [] for m in metrics.keys()} for t in classes} for s in classes} for fe in fe_list}
