"""Image metrics on the device: the squared error, PSNR and SSIM of libngp_metrics.so (include/ngp_metrics.h has the exact
rule), the two metric classes the reference's train.py takes from torchmetrics, and the validation step as a function.

    from ngp_pl_amd import metrics
    metrics.psnr(pred, target)                  # f64 (n,), pred / target (n, h, w, c) or (h, w, c) f32 on the GPU
    metrics.ssim(pred, target, mask=covered)    # the 11-tap Gaussian window over the valid region, per image
    val_psnr = metrics.PeakSignalNoiseRatio(data_range=1)
    val_ssim = metrics.StructuralSimilarityIndexMeasure(data_range=1)

Sums are f64 in an order fixed by the shapes alone: the same inputs give the same 64 bits, with or without a mask.  There is
no CPU or eager fallback: CPU tensors are refused, as `vren.*` refuses them.

`LearnedPerceptualImagePatchSimilarity` is absent: LPIPS is a distance between the activations of a pretrained VGG, and those
weights are not part of this package and cannot be derived; a class of that name with other weights would report numbers that
compare with nobody's.  The reference only builds it under --eval_lpips.
"""
import math

import torch

from . import _metrics_lib as _L
from ._metrics_lib import device_guard, ptr, stream

_LAYOUTS = {"hwc": _L.HWC, "chw": _L.CHW}


def _images(pred, target, mask, layout, min_side):
    """-> contiguous f32 pred, target (4-d), u8 mask or None, (n, c, h, w), whether the leading n was added."""
    if layout not in _LAYOUTS:
        raise ValueError("layout must be 'hwc' or 'chw': %r" % (layout,))
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("pred and target must be tensors")
    if not pred.is_cuda or not target.is_cuda:
        raise RuntimeError("pred and target must be CUDA (HIP) tensors: there is no CPU path")
    if pred.device != target.device:
        raise RuntimeError("pred and target are on different devices")
    if pred.shape != target.shape:
        raise ValueError("pred %r and target %r differ in shape" % (tuple(pred.shape), tuple(target.shape)))
    if not pred.is_floating_point() or not target.is_floating_point():
        raise TypeError("pred and target must be floating point")
    single = pred.dim() == 3
    if pred.dim() not in (3, 4):
        raise ValueError("images must be (n, h, w, c) / (n, c, h, w), or one image without n: %r" % (tuple(pred.shape),))
    if single:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    pred = pred.detach().to(torch.float32).contiguous()
    target = target.detach().to(torch.float32).contiguous()
    n, (c, h, w) = pred.shape[0], ((pred.shape[3], pred.shape[1], pred.shape[2]) if layout == "hwc" else pred.shape[1:])
    if n < 1 or not 1 <= c <= _L.MAX_CHANNELS:
        raise ValueError("need n >= 1 images of 1..4 channels (layout %r): %r" % (layout, tuple(pred.shape)))
    if not (min_side <= h <= _L.MAX_SIDE and min_side <= w <= _L.MAX_SIDE):
        raise ValueError("h and w must be %d..%d: %d x %d" % (min_side, _L.MAX_SIDE, h, w))
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != pred.device:
            raise RuntimeError("mask must be a tensor on the images' device")
        if single and mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if tuple(mask.shape) != (n, h, w):
            raise ValueError("mask must be (n, h, w) = %r: %r" % ((n, h, w), tuple(mask.shape)))
        mask = (mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)).contiguous()
    return pred, target, mask, (n, c, h, w), single


def _workspace(n, c, h, w, dev):
    nbytes = _L.lib().ngp_metrics_workspace_bytes(n, c, h, w)
    if nbytes == 0:
        raise _L.NgpError("ngp_metrics_workspace_bytes: sizes out of range (n=%d c=%d h=%d w=%d)" % (n, c, h, w))
    return torch.empty(nbytes // 8, dtype=torch.int64, device=dev), nbytes


def _sq_error(pred, target, mask, n, c, h, w, layout):
    dev = pred.device
    with device_guard(dev):
        ws, nbytes = _workspace(n, c, h, w, dev)
        total = torch.empty(n, dtype=torch.float64, device=dev)
        count = torch.empty(n, dtype=torch.int64, device=dev)
        _L.call("ngp_metrics_sq_error", ptr(pred), ptr(target), ptr(mask), n, c, h, w, _LAYOUTS[layout], ptr(ws), nbytes, ptr(total), ptr(count), stream())
    return total, count


def _ssim(pred, target, mask, n, c, h, w, layout, data_range, want_map):
    dev = pred.device
    with device_guard(dev):
        ws, nbytes = _workspace(n, c, h, w, dev)
        total = torch.empty(n, dtype=torch.float64, device=dev)
        count = torch.empty(n, dtype=torch.int64, device=dev)
        smap = None
        if want_map:
            smap = torch.empty((n, h - 10, w - 10, c) if layout == "hwc" else (n, c, h - 10, w - 10), dtype=torch.float32, device=dev)
        _L.call("ngp_metrics_ssim", ptr(pred), ptr(target), ptr(mask), n, c, h, w, _LAYOUTS[layout], data_range, ptr(ws), nbytes, ptr(total), ptr(count),
                ptr(smap), stream())
    return total, count, smap


def _data_range(data_range):
    data_range = float(data_range)
    if not (data_range > 0 and math.isfinite(data_range)):
        raise ValueError("data_range must be finite and > 0: %r" % (data_range,))
    return data_range


def sq_error(pred, target, mask=None, layout="hwc"):
    """(sum f64 (n,), count i64 (n,)) of (pred - target)^2 per image, formed in f32 and added in f64; mask (n, h, w) selects
    pixels, and the count is c per selected pixel.  No host sync."""
    pred, target, mask, (n, c, h, w), _ = _images(pred, target, mask, layout, 1)
    return _sq_error(pred, target, mask, n, c, h, w, layout)


def _psnr_of(total, count, data_range):
    """10 log10(data_range^2 / (total / count)) in f64: inf where total is 0, nan where count is 0."""
    return 10.0 * torch.log10(data_range * data_range / (total / count.to(torch.float64)))


def psnr(pred, target, data_range=1.0, mask=None, layout="hwc"):
    """f64 (n,): 10 log10(data_range^2 / mean squared error) per image; inf for identical images, nan where the mask selects
    nothing.  No host sync."""
    data_range = _data_range(data_range)
    total, count = sq_error(pred, target, mask, layout)
    return _psnr_of(total, count, data_range)


def ssim_sums(pred, target, data_range=1.0, mask=None, layout="hwc"):
    """(sum f64 (n,), count i64 (n,)) of the index per image, as sq_error returns its pair: for scores pooled over images, which
    are a ratio of sums and not a mean of ratios.  ssim() is sum / count.  No host sync."""
    data_range = _data_range(data_range)
    pred, target, mask, (n, c, h, w), _ = _images(pred, target, mask, layout, _L.WINDOW_TAPS)
    total, count, _ = _ssim(pred, target, mask, n, c, h, w, layout, data_range, False)
    return total, count


def ssim(pred, target, data_range=1.0, mask=None, layout="hwc", return_map=False):
    """f64 (n,): the mean structural similarity index per image, 11-tap Gaussian window (sigma 1.5) over the valid region, over
    all channels; mask (n, h, w) selects the windows by their centre pixel (nan where it selects none).  return_map=True also
    returns the f32 map, (n, h - 10, w - 10, c) or (n, c, h - 10, w - 10), every window whatever the mask.  No host sync."""
    data_range = _data_range(data_range)
    pred, target, mask, (n, c, h, w), single = _images(pred, target, mask, layout, _L.WINDOW_TAPS)
    total, count, smap = _ssim(pred, target, mask, n, c, h, w, layout, data_range, return_map)
    score = total / count.to(torch.float64)
    if return_map:
        return score, (smap[0] if single else smap)
    return score


class PeakSignalNoiseRatio:
    """torchmetrics' class of this name as train.py uses it: `update` / call with (preds, target) of any shape, `compute` the PSNR
    over everything seen since `reset`.  Squared error and element count accumulate on the device; no host sync."""

    def __init__(self, data_range=1.0):
        self.data_range = _data_range(data_range)
        self.reset()

    def reset(self):
        self.sum_squared_error = None
        self.total = None

    def to(self, *args, **kwargs):
        return self

    @staticmethod
    def _flat(preds, target):
        if preds.shape != target.shape:
            raise ValueError("preds %r and target %r differ in shape" % (tuple(preds.shape), tuple(target.shape)))
        p = preds.detach().to(torch.float32).contiguous().view(-1)
        t = target.detach().to(torch.float32).contiguous().view(-1)
        # as images of one channel: whole blocks of MAX_SIDE x MAX_SIDE, the whole rows of the rest, the last part row
        side, at, numel = _L.MAX_SIDE, 0, p.numel()
        while at < numel:
            left = numel - at
            h, w = (min(left // side, side), side) if left >= side else (1, left)
            yield p[at:at + h * w].view(1, h, w, 1), t[at:at + h * w].view(1, h, w, 1)
            at += h * w

    def _error(self, preds, target):
        total, count = None, None
        for p, t in self._flat(preds, target):
            s, k = sq_error(p, t)
            total, count = (s, k) if total is None else (total + s, count + k)
        if total is None:
            raise ValueError("empty input")
        return total[0], count[0]

    def update(self, preds, target):
        s, k = self._error(preds, target)
        self.sum_squared_error = s if self.sum_squared_error is None else self.sum_squared_error + s
        self.total = k if self.total is None else self.total + k

    def compute(self):
        if self.total is None:
            raise RuntimeError("compute() before any update()")
        return _psnr_of(self.sum_squared_error, self.total, self.data_range)

    def __call__(self, preds, target):
        """Accumulates, and returns the PSNR of this batch alone."""
        s, k = self._error(preds, target)
        self.sum_squared_error = s if self.sum_squared_error is None else self.sum_squared_error + s
        self.total = k if self.total is None else self.total + k
        return _psnr_of(s, k, self.data_range)


class StructuralSimilarityIndexMeasure:
    """torchmetrics' class of this name as train.py uses it: `update` / call with NCHW (preds, target), `compute` the mean of the
    per-image scores seen since `reset`.  No host sync."""

    def __init__(self, data_range=1.0):
        self.data_range = _data_range(data_range)
        self.reset()

    def reset(self):
        self.similarity = None
        self.total = 0

    def to(self, *args, **kwargs):
        return self

    def _scores(self, preds, target):
        if preds.dim() != 4:
            raise ValueError("preds and target must be (N, C, H, W): %r" % (tuple(preds.shape),))
        return ssim(preds, target, self.data_range, layout="chw")

    def _add(self, scores):
        s = scores.sum()
        self.similarity = s if self.similarity is None else self.similarity + s
        self.total += scores.shape[0]

    def update(self, preds, target):
        self._add(self._scores(preds, target))

    def compute(self):
        if self.total == 0:
            raise RuntimeError("compute() before any update()")
        return self.similarity / self.total

    def __call__(self, preds, target):
        """Accumulates, and returns the mean score of this batch alone."""
        scores = self._scores(preds, target)
        self._add(scores)
        return scores.mean()


def evaluate_frames(model, K, poses, img_wh, targets, data_range=1.0, return_frames=False, **render_kwargs):
    """The validation step as a function: per pose get_rays and render(test_time=True), the frame scored against targets[i]
    (H, W, 3).  K (3, 3), poses (C, 3, 4) camera-to-world, img_wh = (W, H).  Returns dict(psnr=[...], ssim=[...], psnr_mean=,
    ssim_mean=) and, with return_frames=True, frames (C, H, W, 3) f32 on the device.  One host read per frame."""
    from .rendering import render
    from .synthetic import get_ray_directions, get_rays
    data_range = _data_range(data_range)
    dev = model.xyz_min.device
    if dev.type != "cuda":
        raise RuntimeError("the model must be on a CUDA (HIP) device")
    K = torch.as_tensor(K).to(dtype=torch.float32)
    poses = torch.as_tensor(poses)[:, :3, :4].to(device=dev, dtype=torch.float32).contiguous()
    W, H = int(img_wh[0]), int(img_wh[1])
    if len(targets) != poses.shape[0]:
        raise ValueError("%d targets for %d poses" % (len(targets), poses.shape[0]))
    dirs = get_ray_directions(H, W, K.cpu(), device=dev)
    frames = torch.empty(poses.shape[0], H, W, 3, dtype=torch.float32, device=dev) if return_frames else None
    psnrs, ssims = [], []
    with torch.no_grad():
        for i in range(poses.shape[0]):
            rays_o, rays_d = get_rays(dirs, poses[i])
            r = render(model, rays_o, rays_d, **dict(render_kwargs, test_time=True))
            frame = r["rgb"].float().view(1, H, W, 3).contiguous()
            target = torch.as_tensor(targets[i]).to(device=dev, dtype=torch.float32).reshape(1, H, W, 3).contiguous()
            both = torch.cat([psnr(frame, target, data_range), ssim(frame, target, data_range)]).tolist()      # the frame's host read
            psnrs.append(both[0])
            ssims.append(both[1])
            if return_frames:
                frames[i] = frame[0]
    out = dict(psnr=psnrs, ssim=ssims, psnr_mean=sum(psnrs) / len(psnrs), ssim_mean=sum(ssims) / len(ssims))
    if return_frames:
        out["frames"] = frames
    return out
