"""ngp_hashgrid_bwd_binned against the exact integer reference (tests/table_backward_reference.py).

The kernel's contract: every table entry is an exact 64-bit fixed-point sum in 2^-24 units, written out as
f16(clip(f32(sum) * 2^-24, +-65504)).  So on every level that one task per slice writes (all hashed levels) the result is compared
BIT FOR BIT.  The dense levels are summed in K <= 16 parts whose f32 partial tables merge_kernel adds in f32; there the bound is

    |got - clip(Q * 2^-24)| <= 1/2 ulp16(got) + 2^-19 * M_e,      M_e = sum |q| * 2^-24 of the entry

derived, not measured: each part's integer sum is rounded once to f32 (<= 2^-24 of the part's mass), the K - 1 f32 additions round
once each (<= 2^-24 of the mass so far), 2 K <= 32 roundings of at most 2^-24 M_e in all; the final f16 conversion adds half an ulp,
and the clamp to +-65504 moves nothing apart.  Which levels are dense is read from the level table (res^3 <= size), not from the
kernel.  That the inputs reach the paths they are built for is asserted in tests/test_table_backward_reference_cpu.py on the same
cached cases, and again here where a test depends on it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import table_backward_cases as K
from tests import table_backward_reference as R

pytestmark = pytest.mark.gpu

SMALL_N = (0, 1, 63, 1023, 1024, 1025, 3079)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def run_binned(lib, case, x, d, n_samples, active=None, n_active=None, groups=1, ws=None, out=None):
    """One table backward into a NaN-filled table (or `out`); returns the table on the host as numpy f16."""
    grid, meta = case.grid, case.meta
    xs, dfl = x.cuda().contiguous(), d.cuda().contiguous()
    mnt, mxt = torch.from_numpy(grid.xyz_min).cuda(), torch.from_numpy(grid.xyz_max).cuda()
    act = None if active is None else active.cuda()
    nact = None if n_active is None else torch.tensor([n_active], dtype=torch.int32, device="cuda")
    nbytes = lib.lib().ngp_hashgrid_bwd_binned_workspace_bytes(C.byref(meta), n_samples)
    assert nbytes > 0
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert ws.numel() >= nbytes
    grad = torch.full((grid.offset[-1], 2), float("nan"), dtype=torch.float16, device="cuda") if out is None else out
    if groups == 1:
        lib.call("ngp_hashgrid_bwd_binned", lib.ptr(xs), lib.ptr(mnt), lib.ptr(mxt), lib.ptr(dfl), C.byref(meta), n_samples, lib.ptr(act), lib.ptr(nact),
                 lib.ptr(ws), nbytes, lib.ptr(grad), lib.stream())
    else:
        for grp in range(groups):
            lib.call("ngp_hashgrid_bwd_binned_group", lib.ptr(xs), lib.ptr(mnt), lib.ptr(mxt), lib.ptr(dfl), C.byref(meta), n_samples, lib.ptr(act), lib.ptr(nact),
                     lib.ptr(ws), nbytes, lib.ptr(grad), groups, grp, lib.stream())
    torch.cuda.synchronize()
    return grad.cpu().numpy()


def check(got, ref, grid, what=""):
    assert not np.isnan(got.astype(np.float32)).any(), "%s: entries left unwritten" % what
    assert np.isfinite(got.astype(np.float32)).all(), "%s: inf" % what
    for l in range(grid.n_levels):
        a, b = grid.offset[l], grid.offset[l + 1]
        g, want = got[a:b], ref.f16_exact[a:b]
        if ref.hashed[l]:
            # bit for bit (stricter than ==: the sign of a zero counts too)
            diff = g.view(np.int16) != want.view(np.int16)
            if diff.any():
                e, k = np.argwhere(diff)[0]
                lv = ref.levels[l] if ref.levels else None
                who = [] if lv is None else sorted(set(int(j) for c in range(8) for j in lv.j[lv.idx[c] == e]))[:12]
                raise AssertionError("%s: level %d (hashed, res %d): %d of %d values differ; first entry %d feature %d: got %r, exact %r, Q %d, n_e %d, live columns %r" % (
                    what, l, grid.resolution[l], int(diff.sum()), diff.size, e, k, float(g[e, k]), float(want[e, k]), int(ref.Q[a + e, k]), int(ref.n_e[a + e]), who))
        else:
            exact = np.clip(ref.Q[a:b].astype(np.float64) / R.FIX_ONE, -R.F16_MAX, R.F16_MAX)
            err = np.abs(g.astype(np.float64) - exact)
            bound = 0.5 * R.ulp16(g) + 2.0 ** -19 * ref.M_e[a:b]
            bad = err > bound
            if bad.any():
                e, k = np.argwhere(bad)[0]
                raise AssertionError("%s: level %d (dense, res %d): %d of %d values out of bound; first entry %d feature %d: got %r, exact %r, bound %g, mass %g, n_e %d" % (
                    what, l, grid.resolution[l], int(bad.sum()), bad.size, e, k, float(g[e, k]), float(exact[e, k]), float(bound[e, k]), float(ref.M_e[a + e, k]), int(ref.n_e[a + e])))
            assert not g[ref.n_e[a:b] == 0].any(), "%s: level %d: an entry nothing reaches is not zero" % (what, l)


@pytest.mark.parametrize("name,n", [("small", n) for n in SMALL_N] + [("product", 20011), ("scale16", 20011)])
def test_binned_backward_is_the_exact_sum(lib, name, n):
    c = K.plain_case(name, n)
    if name == "small":
        assert K.dense_split_branches(c.grid) == (True, True, True) and K.has_partial_last_slice(c.grid)
    else:
        assert K.straddling_pairs(c.ref) >= 20
    if n >= 63:
        assert K.seeds_cover_the_range(c.d)
    got = run_binned(lib, c, c.x, c.d, n)
    check(got, c.ref, c.grid, "%s n=%d" % (name, n))
    if n == 0:
        assert not got.view(np.int16).any()                             # success, and an all-zero table
    else:
        assert got.any()


@pytest.mark.parametrize("big", [False, True])
def test_many_samples_of_one_block_in_one_cell(lib, big):
    """4096 points in one finest-level cell: a hashed entry takes > 512 contributions from one block of samples (segments longer than
    one wave pass) and every dense level sees one long run.  big: every gradient +60 000 -- sums leave the f16 range and must come
    out as exactly +65504, never inf."""
    c = K.crowd_case("small", 4096, big)
    assert K.max_contributions_of_one_block(c.ref) > 512 and K.dense_levels_hold_one_cell(c.ref)
    got = run_binned(lib, c, c.x, c.d, 4096)
    check(got, c.ref, c.grid, "crowd big=%s" % big)
    if big:
        over = c.ref.Q.astype(np.float64) / R.FIX_ONE > R.F16_MAX
        assert over.any() and (got[over] == np.float16(65504.0)).all()


@pytest.mark.parametrize("name,n", [("small", 3079), ("product", 20011)])
def test_live_prefix_and_indirection(lib, name, n):
    """What the trainer runs: dfeats in compact order with the live count on the device, with and without the index list."""
    c = K.plain_case(name, n)
    m = (2 * n) // 5
    act = K.make_active(n, m, seed=31)
    pad = torch.full((n - m,), -1, dtype=torch.int32)
    d_compact = torch.full_like(c.d, 7.0)                               # columns past the live prefix are never read
    d_compact[:, :m] = c.d[:, act.long()]
    # (1) index list + live count
    a1 = torch.cat([act, pad])
    check(run_binned(lib, c, c.x, d_compact, n, a1, m), K.reference_of(c.grid, c.x, d_compact, a1, m), c.grid, "%s active_idx" % name)
    # (2) live count alone: x compact as well
    x_compact = c.x.clone()
    x_compact[:m] = c.x[act.long()]
    ref2 = K.reference_of(c.grid, x_compact, d_compact, None, m)
    assert np.array_equal(ref2.Q, K.reference_of(c.grid, c.x, d_compact, a1, m).Q)
    check(run_binned(lib, c, x_compact, d_compact, n, None, m), ref2, c.grid, "%s n_active alone" % name)
    # (3) nothing live
    got = run_binned(lib, c, c.x, d_compact, n, torch.full((n,), -1, dtype=torch.int32), 0)
    assert not got.view(np.int16).any()
    # (4) a count past the batch is clamped to it; the list's entries behind the live prefix are -1
    x_more = K.make_points(n + 500, c.grid.half, seed=32)
    a4 = torch.cat([K.make_active(n + 500, n, seed=33), torch.full((5,), -1, dtype=torch.int32)])
    check(run_binned(lib, c, x_more, c.d, n, a4, n + 5), K.reference_of(c.grid, x_more, c.d, a4, n + 5), c.grid, "%s clamped count" % name)


def test_two_calls_on_one_uninitialised_workspace_agree(lib):
    c = K.plain_case("small", 3079)
    nbytes = lib.lib().ngp_hashgrid_bwd_binned_workspace_bytes(C.byref(c.meta), 3079)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    first = run_binned(lib, c, c.x, c.d, 3079, ws=ws)
    second = run_binned(lib, c, c.x, c.d, 3079, ws=ws)
    assert np.array_equal(first.view(np.int16), second.view(np.int16))
    check(second, c.ref, c.grid, "second call")


def test_three_launch_groups_give_the_exact_sums(lib):
    c = K.plain_case("small", 3079)
    check(run_binned(lib, c, c.x, c.d, 3079, groups=3), c.ref, c.grid, "3 groups")
