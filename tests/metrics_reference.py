"""Test infrastructure (no GPU): include/ngp_metrics.h restated three ways.

  ssim_f32      THE RULE in numpy float32, operation by operation: rows then columns, taps in order, products before the
                filter, no fused multiply-add (numpy rounds every ufunc once).  Returns the map, the sums by math.fsum of the
                selected entries (the correctly rounded sum, which any order of f64 additions approaches) and the counts.
  ssim_f64      the definition in float64: a direct 121-tap two-dimensional Gaussian window over the valid region.
  ssim_torch    the statement in torch: reflection pad 5, one grouped F.conv2d with the outer-product kernel over the five
                stacked maps, crop 5 (which leaves the valid region).
  sq_error_f32  the squared error likewise, and sq_error_f64.

Images are (n, h, w, c) for layout "hwc" and (n, c, h, w) for "chw"; maps come back in the layout of the input.
"""
import math

import numpy as np

F = np.float32
TAPS, HALO = 11, 10


def window64():
    k = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-((k - 5.0) / 1.5) ** 2 / 2.0)
    return g / g.sum()


def window():
    """The eleven weights: the formula in f64, rounded to f32 once."""
    return window64().astype(F)


def constants(data_range):
    dr = float(data_range)
    return F((0.01 * dr) * (0.01 * dr)), F((0.03 * dr) * (0.03 * dr))


def planar(a, layout):
    a = np.asarray(a)
    if layout == "hwc":
        return np.ascontiguousarray(np.moveaxis(a, -1, -3))
    if layout == "chw":
        return np.ascontiguousarray(a)
    raise ValueError(layout)


def _as_layout(m, layout):
    return np.ascontiguousarray(np.moveaxis(m, -3, -1)) if layout == "hwc" else m


def filter_f32(m):
    """(..., h, w) f32 -> (..., h - 10, w - 10): the row pass, then the column pass over its result."""
    g = window()
    m = np.asarray(m, F)
    w = m.shape[-1] - HALO
    a = g[0] * m[..., :, 0:w]
    for k in range(1, TAPS):
        a = a + g[k] * m[..., :, k:k + w]
    h = a.shape[-2] - HALO
    b = g[0] * a[..., 0:h, :]
    for k in range(1, TAPS):
        b = b + g[k] * a[..., k:k + h, :]
    assert b.dtype == F
    return b


def index_f32(mp, mt, pp, tt, pt, c1, c2):
    two = F(2)
    spp = pp - mp * mp
    stt = tt - mt * mt
    spt = pt - mp * mt
    num = ((two * mp) * mt + c1) * (two * spt + c2)
    den = ((mp * mp + mt * mt) + c1) * ((spp + stt) + c2)
    s = num / den
    assert s.dtype == F
    return s


def centre_mask(mask, n, h, w):
    """(n, h - 10, w - 10) bool: the window's centre pixel is selected."""
    if mask is None:
        return np.ones((n, h - HALO, w - HALO), bool)
    return np.asarray(mask).reshape(n, h, w)[:, 5:h - 5, 5:w - 5] != 0


def _reduce(smap, sel):
    """smap (n, c, oh, ow), sel (n, oh, ow) -> fsum per image over the selected windows and all channels, counts."""
    n, c = smap.shape[:2]
    sums = [math.fsum(smap[i][:, sel[i]].astype(np.float64).ravel().tolist()) for i in range(n)]
    counts = [int(sel[i].sum()) * c for i in range(n)]
    return sums, counts


def ssim_f32(pred, target, data_range=1.0, mask=None, layout="hwc"):
    p, t = planar(pred, layout).astype(F), planar(target, layout).astype(F)
    n, c, h, w = p.shape
    c1, c2 = constants(data_range)
    with np.errstate(all="ignore"):
        s = index_f32(filter_f32(p), filter_f32(t), filter_f32(p * p), filter_f32(t * t), filter_f32(p * t), c1, c2)
    sums, counts = _reduce(s, centre_mask(mask, n, h, w))
    return _as_layout(s, layout), sums, counts


def ssim_f64(pred, target, data_range=1.0, layout="hwc"):
    """The map of the definition in float64 (planar inputs widened, a direct 121-tap window), in the input's layout."""
    p, t = planar(pred, layout).astype(np.float64), planar(target, layout).astype(np.float64)
    g = window64()
    k2 = np.outer(g, g)
    h, w = p.shape[-2] - HALO, p.shape[-1] - HALO

    def filt(m):
        out = np.zeros(m.shape[:-2] + (h, w))
        for dy in range(TAPS):
            for dx in range(TAPS):
                out += k2[dy, dx] * m[..., dy:dy + h, dx:dx + w]
        return out

    dr = float(data_range)
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    mp, mt, pp, tt, pt = filt(p), filt(t), filt(p * p), filt(t * t), filt(p * t)
    spp, stt, spt = pp - mp * mp, tt - mt * mt, pt - mp * mt
    s = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    return _as_layout(s, layout)


def ssim_torch(pred, target, data_range=1.0, layout="hwc"):
    """The torch statement, float32 on the tensors' device; returns the map as a numpy array in the input's layout."""
    import torch
    import torch.nn.functional as Fn
    p = torch.as_tensor(pred, dtype=torch.float32)
    t = torch.as_tensor(target, dtype=torch.float32)
    if layout == "hwc":
        p, t = p.movedim(-1, -3), t.movedim(-1, -3)
    n, c, h, w = p.shape
    g = torch.from_numpy(window()).to(p.device)
    kernel = torch.outer(g, g).expand(5 * c, 1, TAPS, TAPS).contiguous()
    stack = torch.cat([p, t, p * p, t * t, p * t], dim=1)
    out = Fn.conv2d(Fn.pad(stack, (5, 5, 5, 5), mode="reflect"), kernel, groups=5 * c)[..., 5:-5, 5:-5]
    mp, mt, pp, tt, pt = out.split(c, dim=1)
    c1, c2 = (float(x) for x in constants(data_range))
    spp, stt, spt = pp - mp * mp, tt - mt * mt, pt - mp * mt
    s = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    if layout == "hwc":
        s = s.movedim(-3, -1)
    return s.contiguous().cpu().numpy()


def pixel_mask(mask, n, h, w):
    if mask is None:
        return np.ones((n, h, w), bool)
    return np.asarray(mask).reshape(n, h, w) != 0


def sq_error_f32(pred, target, mask=None, layout="hwc"):
    """d = p - t and d * d in f32, widened; fsum per image over the selected pixels and all channels, counts."""
    p, t = planar(pred, layout).astype(F), planar(target, layout).astype(F)
    n, c, h, w = p.shape
    d = p - t
    e = d * d
    assert e.dtype == F
    return _reduce(e, pixel_mask(mask, n, h, w))


def sq_error_f64(pred, target, mask=None, layout="hwc"):
    p, t = planar(pred, layout).astype(np.float64), planar(target, layout).astype(np.float64)
    n, c, h, w = p.shape
    return _reduce((p - t) ** 2, pixel_mask(mask, n, h, w))


def psnr(total, count, data_range=1.0):
    """10 log10(data_range^2 / (total / count)): inf where total is 0, nan where count is 0."""
    if count == 0:
        return float("nan")
    if total == 0:
        return float("inf")
    return 10.0 * math.log10(float(data_range) ** 2 / (total / count))


def mean(total, count):
    return total / count if count else float("nan")


# ---- the input classes of the GPU tests (seeded), (n, h, w, c) f32 and the data_range each is scored with


CLASSES = ("noise", "smooth", "flat", "quantised", "white", "range4")


def images(kind, n, h, w, c, seed=0):
    """pred, target (n, h, w, c) f32 and data_range."""
    g = np.random.RandomState(seed + 1000 * CLASSES.index(kind))
    shape = (n, h, w, c)
    if kind == "noise":
        return g.rand(*shape).astype(F), g.rand(*shape).astype(F), 1.0
    if kind in ("smooth", "quantised"):
        y, x = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.4 * np.sin(x / 7.0)[None, :, :, None] * np.cos(y / 5.0)[None, :, :, None] + 0.02 * np.arange(c)[None, None, None, :]
        p = np.clip(base + 0.05 * g.randn(*shape), 0, 1)
        t = np.clip(base + 0.05 * g.randn(*shape), 0, 1)
        if kind == "quantised":
            p, t = np.round(p * 255) / 255, np.round(t * 255) / 255
        return p.astype(F), t.astype(F), 1.0
    if kind == "flat":
        return (0.5 + 1e-3 * g.randn(*shape)).astype(F), (0.5 + 1e-3 * g.randn(*shape)).astype(F), 1.0
    if kind == "white":
        return np.ones(shape, F), np.ones(shape, F), 1.0
    if kind == "range4":
        return (4 * g.rand(*shape)).astype(F), (4 * g.rand(*shape)).astype(F), 4.0
    raise ValueError(kind)


def cases(tile_w, tile_h):
    """The (kind, n, h, w, c, layout) of the map tests: h and w from {11, 12, 21} and {T - 1, T, T + 1, 2 T + 1} + 10 for the
    tile's T along each axis, every pair once; classes, channels, layouts and batch sizes rotate through them."""
    hs = [11, 12, 21] + [t + 10 for t in (tile_h - 1, tile_h, tile_h + 1, 2 * tile_h + 1)]
    ws = [11, 12, 21] + [t + 10 for t in (tile_w - 1, tile_w, tile_w + 1, 2 * tile_w + 1)]
    out, k = [], 0
    for h in hs:
        for w in ws:
            out.append((CLASSES[k % 6], 3 if k % 5 == 0 else 1, h, w, (1, 3, 4)[(k // 6) % 3], ("hwc", "chw")[(k // 18 + k) % 2]))
            k += 1
    return out


def case_images(case, seed=0):
    """pred, target in the case's layout, and data_range."""
    kind, n, h, w, c, layout = case
    p, t, dr = images(kind, n, h, w, c, seed)
    if layout == "chw":
        p, t = np.ascontiguousarray(np.moveaxis(p, -1, 1)), np.ascontiguousarray(np.moveaxis(t, -1, 1))
    return p, t, dr
