"""ngp_hashgrid_fwd / _fwd_n / _fwd_list and ngp_hashgrid_bwd_input against the exact reference (tests/hashgrid_forward_reference.py).

Every output is held to its own derived limit (the reference's docstring has the derivation):

    forward:        |out - exact| <= gamma_11 * mass + 1/2 ulp16(|exact| + gamma_11 * mass)
    input gradient: |out_k - grad_k| <= gamma_32 * mass_k

with the kernel's own cell, bit for bit, so samples ON cell faces, at the box corners and outside the box are held like any other: no
sample is filtered out.  Output buffers are prefilled with a NaN bit pattern and carry a guard band: every element that should be
written must be written (a NaN is out of every limit) and nothing else may change.  That the inputs reach the paths they are built for
(cell runs across wave boundaries, faces, both out-of-box directions on dense and hashed levels, ...) is asserted on the CPU in
tests/test_hashgrid_forward_reference_cpu.py on the same cases, where five wrong kernels are also shown to fail the check used here.

BIT EQUALITY WITH THE EMULATION.  The reference also emulates the kernel's operation order (f32 weights ((wx wy) wz), eight fmafs from
c = 0, one conversion to f16).  The share of forward outputs whose 16 bits equal it is computed and printed for every case.  OUTCOME of
the first run on an MI355X: 100 % on every one of the 307 cases of this file (every point set x grid x box x table, every count, the
device-sized and the list launches; 7.8 M outputs, the sign of a zero included).  So equality is ASSERTED from then on (PIN_EMULATED):
the forward's arithmetic is pinned like the marcher's, and a rewrite that reorders the eight fmafs, drops the fmaf in pos or converts
twice fails here even where it stays inside the limit.  The limit stays asserted as well: it is what holds the emulation itself to the
exact value.  (The 99.98 % of tests/test_hashgrid_forward_reference_cpu.py is another figure: the emulation against f16(exact).)
The input gradient's file is compiled with contraction allowed and has no emulation; the kernel used less than a tenth of its limit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import hashgrid_forward_cases as H
from tests import hashgrid_forward_reference as F

pytestmark = pytest.mark.gpu

# True (since the first run gave 100 % everywhere): every forward output must equal the emulation bit for bit.
PIN_EMULATED = True

PREFILL16, PREFILL32 = 0x7E5A, 0x7FC5A5A5      # NaN bit patterns (f16, f32)
GUARD = 4096
_TABLES = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def dev_table(name, kind):
    if (name, kind) not in _TABLES:
        _TABLES[(name, kind)] = torch.from_numpy(H.table_of(name, kind)).cuda()
    return _TABLES[(name, kind)]


def dev_box(name, box):
    mn, mx = H.box_of(H.grid_of(name)[0], box)
    return torch.from_numpy(mn).cuda(), torch.from_numpy(mx).cuda()


def prefilled(numel):
    return torch.full((numel + GUARD,), PREFILL16, dtype=torch.int16, device="cuda")


def written(buf, n_levels, n):
    """The host copy of an output buffer: its first n_levels * n * 2 values as (L, n, 2) f16; asserts that nothing behind them changed."""
    host = buf.cpu().numpy()
    m = n_levels * n * 2
    assert (host[m:] == PREFILL16).all(), "%d values written behind the %d x %d outputs" % (int((host[m:] != PREFILL16).sum()), n_levels, n)
    return host[:m].view(np.float16).reshape(n_levels, n, 2)


def hold(got, ref, what, rows=None):
    bad, worst, _ = F.out_of_limit(got, ref, rows)
    share = F.share_equal(got, ref, rows)
    print("%-60s %8d outputs, %.4f %% equal the emulation; %s" % (what, got.size, 100.0 * share, worst))
    assert bad == 0, "%s: %d of %d outputs out of limit; %s" % (what, bad, got.size, worst)
    if PIN_EMULATED:
        emu = ref.emulated if rows is None else ref.emulated[:, rows]
        assert np.array_equal(got.view(np.int16), emu.view(np.int16)), "%s: %d outputs differ from the emulation" % (what, int((got.view(np.int16) != emu.view(np.int16)).sum()))
    return share


def run_fwd(lib, name, box, x, kind, count=None, bound=None):
    """ngp_hashgrid_fwd of x (n, 3), or ngp_hashgrid_fwd_n with launch bound `bound` and device count `count`.  Returns the raw buffer."""
    grid, meta = H.grid_of(name)
    xs = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    mn, mx = dev_box(name, box)
    n = x.shape[0] if bound is None else bound
    out = prefilled(grid.n_levels * n * 2)
    if bound is None:
        lib.call("ngp_hashgrid_fwd", lib.ptr(xs), lib.ptr(mn), lib.ptr(mx), lib.ptr(dev_table(name, kind)), C.byref(meta), n, lib.ptr(out), lib.stream())
    else:
        n_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
        lib.call("ngp_hashgrid_fwd_n", lib.ptr(xs), lib.ptr(mn), lib.ptr(mx), lib.ptr(dev_table(name, kind)), C.byref(meta), n, lib.ptr(n_dev), lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("box", H.BOX_NAMES)
@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_forward_of_every_point_set(lib, name, box):
    grid = H.grid_of(name)[0]
    print()
    for kind in H.TABLE_NAMES:
        for which in H.SET_NAMES:
            ref = H.reference_of(name, box, which, kind)
            got = written(run_fwd(lib, name, box, H.points_of(name, box, which), kind), grid.n_levels, ref.n)
            hold(got, ref, "fwd %s %s %s %s" % (name, box, which, kind))


@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_forward_of_every_count(lib, name):
    """Prefixes of the march-like rays: below a wave, around a wave and a workgroup, several workgroups, a last sample alone in its
    cell and a last run cut in the middle of a wave."""
    grid = H.grid_of(name)[0]
    ref = H.reference_of(name, "sym", "march", "uniform")
    x = H.points_of(name, "sym", "march")
    print()
    for n in H.counts_of(ref):
        got = written(run_fwd(lib, name, "sym", x[:n], "uniform"), grid.n_levels, n)
        hold(got, ref, "fwd %s n=%d" % (name, n), np.arange(n))


@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_device_sized_forward(lib, name):
    """ngp_hashgrid_fwd_n: the launch covers a bound S, the count comes from device memory and is also the level stride of the
    output (min(count, S)).  Nothing is written for a count of 0, nor behind n_levels * count entries."""
    grid = H.grid_of(name)[0]
    ref = H.reference_of(name, "sym", "march", "uniform")
    x = H.points_of(name, "sym", "march")
    S = ref.n
    print()
    for count in (0, 1, 255, 256, 257, S - 777, S, S + 5):
        n = min(count, S)
        got = written(run_fwd(lib, name, "sym", x, "uniform", count=count, bound=S), grid.n_levels, n)
        hold(got, ref, "fwd_n %s S=%d count=%d" % (name, S, count), np.arange(n))


def run_list(lib, name, box, which, kind, ids, n_list_max, count=None):
    grid, meta = H.grid_of(name)
    x = H.points_of(name, box, which)
    n = x.shape[0]
    xs = torch.from_numpy(x).cuda()
    mn, mx = dev_box(name, box)
    lst = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    assert lst.numel() >= n_list_max
    n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    out = prefilled(grid.n_levels * n * 2)
    lib.call("ngp_hashgrid_fwd_list", lib.ptr(xs), lib.ptr(mn), lib.ptr(mx), lib.ptr(dev_table(name, kind)), C.byref(meta), n, lib.ptr(lst), n_list_max,
             lib.ptr(n_dev), lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    return written(out, grid.n_levels, n)


def hold_list(got, ref, listed, what, ref_rows=None):
    """Listed samples within their limit; every other sample keeps the prefill."""
    n = got.shape[1]
    rest = np.ones(n, bool)
    rest[listed] = False
    assert (got[:, rest].view(np.int16) == PREFILL16).all(), "%s: samples that are not listed were written" % what
    hold(got[:, listed], ref, what, listed if ref_rows is None else ref_rows)


@pytest.mark.parametrize("name", ["product", "levels12", "levels4"])
def test_forward_over_a_sample_list(lib, name):
    print()
    # runs of 7 consecutive samples, every other run
    ref = H.reference_of(name, "sym", "march", "uniform")
    ids = np.arange(ref.n // 7 * 7, dtype=np.int32).reshape(-1, 7)[::2].reshape(-1)
    hold_list(run_list(lib, name, "sym", "march", "uniform", ids, ids.size), ref, ids, "list %s runs of 7" % name)
    # a device count below the host bound: the entries behind it are not read
    m = ids.size // 3
    poisoned = ids.copy()
    poisoned[m:] = ids[m:][::-1]
    hold_list(run_list(lib, name, "sym", "march", "uniform", poisoned, ids.size, count=m), ref, ids[:m], "list %s device count %d of %d" % (name, m, ids.size))
    hold_list(run_list(lib, name, "sym", "march", "uniform", ids, ids.size, count=0), ref, ids[:0], "list %s device count 0" % name)
    hold_list(run_list(lib, name, "sym", "march", "uniform", ids, ids.size, count=ids.size + 9), ref, ids, "list %s device count past the bound" % name)
    # -1 and ids past the end between valid ids of ONE cell (300 samples of one point), and between march samples
    for which in ("repeat", "march"):
        ref = H.reference_of(name, "skew", which, "log")
        n = ref.n
        listed = np.arange(n // 2, dtype=np.int32)                     # the first half of the samples; the other half stays unlisted
        ids = []
        for i in listed.tolist():
            ids += [i] + [[-1], [n + i % 5], [], [2 ** 31 - 1, -1], [], [n], [-1, -1, -1], []][i % 8]
        ids = np.array(ids, np.int32)
        assert ((ids < 0) | (ids >= n)).sum() > listed.size // 2
        hold_list(run_list(lib, name, "skew", which, "log", ids, ids.size), ref, listed, "list %s %s with -1 and ids past the end" % (name, which))


def test_forward_over_a_list_longer_than_the_launch(lib):
    """33 000 ids over 40 000 samples: more than 128 chunks of 256, so the chunks' stride loop runs a second time for some of them."""
    name = "product"
    n = H.points_of(name, "sym", "march_long").shape[0]
    assert n == 40000
    ids = np.sort(np.random.RandomState(9).choice(n, 33000, replace=False)).astype(np.int32)
    assert ids.size > 128 * H.CHUNK
    ref = H.reference_rows(name, "sym", "march_long", "uniform", ids)
    print()
    hold_list(run_list(lib, name, "sym", "march_long", "uniform", ids, ids.size), ref, ids, "list product 33000 of 40000", ref_rows=np.arange(ids.size))


@pytest.mark.parametrize("box", H.BOX_NAMES)
@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_input_gradient(lib, name, box):
    """ngp_hashgrid_bwd_input on the face, ray and out-of-box sets (faces included: the kernel differentiates its own cell's piece, and
    so does the reference), out_scale 1 and 4."""
    grid, meta = H.grid_of(name)
    mn_h, mx_h = H.box_of(grid, box)
    mn, mx = dev_box(name, box)
    table = H.table_of(name, "uniform")
    rng = np.random.RandomState(21)
    print()
    for which in ("faces", "march", "outside"):
        x = H.points_of(name, box, which)[:1030]
        n = x.shape[0]
        d = (rng.randn(grid.n_levels, n, 2) * 0.05).astype(np.float16)
        d[:, ::7] = 0
        xs, ds = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(d).cuda()
        for out_scale in (1.0, 4.0):
            ref = F.input_gradient_reference(x, mn_h, mx_h, table, d, grid.resolution, grid.offset, grid.scale, grid.n_levels, out_scale)
            out = torch.full((3 * n + GUARD,), PREFILL32, dtype=torch.int32, device="cuda")
            lib.call("ngp_hashgrid_bwd_input", lib.ptr(xs), lib.ptr(mn), lib.ptr(mx), lib.ptr(dev_table(name, "uniform")), lib.ptr(ds), C.byref(meta), n,
                     out_scale, lib.ptr(out), lib.stream())
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            assert (host[3 * n:] == PREFILL32).all()
            got = host[:3 * n].view(np.float32).reshape(n, 3).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(got - ref.grad)
                ratio = np.where(np.isfinite(got), np.where(err == 0, 0.0, err / ref.limit), np.inf)
            i, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            what = "bwd_input %s %s %s out_scale %g: worst error/limit %.4f at sample %d axis %d: got %r, exact %r, limit %.3g" % (
                name, box, which, out_scale, float(ratio[i, k]), i, k, float(got[i, k]), float(ref.grad[i, k]), float(ref.limit[i, k]))
            print(what)
            assert (ratio <= 1.0).all(), what
            assert np.abs(ref.grad).max() > 0
