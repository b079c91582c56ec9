"""Times of ngp_pl_amd.metrics.ssim and sq_error on the GPU, for one `--size`^2 x 3 frame and for a batch of `--batch` such frames
(channel-last, uniform noise, seeded), beside the torch statement of SSIM (tests/metrics_reference.py: reflection pad, one grouped
conv2d with the outer-product kernel over the five stacked maps, crop) on the same tensors.  HIP events around `--calls` calls
in a row after a warm-up, the median over `--reps` such windows, per call.  Prints one JSON line: the times, the bytes each call
has to move once (both inputs), that over the time as a rate and as a share of `--peak-tbs` TB/s, and the largest difference
between the library's mean score and the torch statement's.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import metrics
from tests import metrics_reference as R


def timed(fn, calls, reps):
    """Median over reps of (HIP-event time of `calls` calls in a row) / calls, in seconds; two warm-up calls first."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / calls)
    return statistics.median(out), min(out), max(out)


def torch_statement(p, t):
    """Mean score per image of the torch statement on device tensors (n, h, w, 3)."""
    import torch.nn.functional as Fn
    c = p.shape[-1]
    p, t = p.movedim(-1, 1), t.movedim(-1, 1)
    g = torch.from_numpy(R.window()).to(p.device)
    kernel = torch.outer(g, g).expand(5 * c, 1, 11, 11).contiguous()
    out = Fn.conv2d(Fn.pad(torch.cat([p, t, p * p, t * t, p * t], dim=1), (5, 5, 5, 5), mode="reflect"), kernel, groups=5 * c)[..., 5:-5, 5:-5]
    mp, mt, pp, tt, pt = out.split(c, dim=1)
    c1, c2 = (float(x) for x in R.constants(1.0))
    spp, stt, spt = pp - mp * mp, tt - mt * mt, pt - mp * mt
    s = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    return s.double().mean(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window of the single frame (the batch takes a tenth)")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak in TB/s for the share")
    ap.add_argument("--skip-torch-batch", action="store_true", help="time the torch statement on the single frame only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a GPU"
    torch.manual_seed(0)
    res = dict(size=a.size, batch=a.batch, reps=a.reps)
    for name, n, calls in (("frame", 1, a.calls), ("batch", a.batch, max(1, a.calls // 10))):
        p = torch.rand(n, a.size, a.size, 3, device="cuda")
        t = (p + 0.05 * torch.randn_like(p)).clamp(0, 1)
        nbytes = 2 * p.numel() * 4
        rows = [("ssim", lambda: metrics.ssim(p, t)), ("ssim_with_map", lambda: metrics.ssim(p, t, return_map=True)), ("sq_error", lambda: metrics.sq_error(p, t))]
        if name == "frame" or not a.skip_torch_batch:
            rows.append(("ssim_torch_statement", lambda: torch_statement(p, t)))
        for what, fn in rows:
            med, lo, hi = timed(fn, calls, a.reps)
            res["%s_%s_s" % (name, what)] = med
            res["%s_%s_min_max_s" % (name, what)] = (lo, hi)
            if what != "ssim_torch_statement":
                res["%s_%s_share_of_hbm_peak" % (name, what)] = nbytes / med / (a.peak_tbs * 1e12)
        res["%s_input_bytes" % name] = nbytes
        if name == "frame" or not a.skip_torch_batch:
            res["%s_max_abs_difference_to_torch_statement" % name] = float((metrics.ssim(p, t) - torch_statement(p, t)).abs().max().item())
        del p, t
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
