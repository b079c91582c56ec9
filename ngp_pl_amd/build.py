"""Builds the native pieces in-tree (no JIT cache, so the .so files travel with the repo snapshot).

  libngp_hip.so   -- the product: hand-written HIP kernels for gfx950 behind the C ABI of
                     include/ngp_hip.h.  hipcc cross-compiles without a GPU.
  libngp_mesh.so  -- mesh export (marching cubes over a density volume) behind include/ngp_mesh.h; its sources
                     live under csrc/mesh/, apart from SOURCES.
  libngp_meshfilter.so -- connected components and component filtering of a mesh behind include/ngp_meshfilter.h; its
                     sources live under csrc/meshfilter/.
  libngp_meshcull.so -- depth-buffer visibility of a mesh against cameras and the cull of unseen faces behind
                     include/ngp_meshcull.h; its sources live under csrc/meshcull/.  The order-preserving compaction
                     (csrc/mesh_compact.h) is shared source of this library, the component filter, the simplifier and the
                     decimator.
  libngp_meshsimplify.so -- simplification of a mesh by vertex clustering behind include/ngp_meshsimplify.h; its sources
                     live under csrc/meshsimplify/.
  libngp_meshtsdf.so -- fusion of per-camera depth maps into a truncated signed distance volume on the export lattice behind
                     include/ngp_meshtsdf.h; its sources live under csrc/meshtsdf/.
  libngp_meshsmooth.so -- Taubin smoothing of a mesh on an integer grid and geometric vertex normals behind
                     include/ngp_meshsmooth.h; its sources live under csrc/meshsmooth/.
  libngp_meshtex.so -- the texture atlas of a mesh (layout, texel points, UVs) and the renderer of the textured mesh behind
                     include/ngp_meshtex.h; its sources live under csrc/meshtex/.
  libngp_metrics.so -- image metrics (the squared error behind PSNR, and SSIM with the Gaussian window) behind
                     include/ngp_metrics.h; its sources live under csrc/metrics/.
  libngp_meshdist.so -- the geometric distance between two meshes (surface samples, the nearest face through a uniform grid,
                     the weighted statistics behind Chamfer, Hausdorff and F-score) behind include/ngp_meshdist.h; its sources
                     live under csrc/meshdist/.
  libngp_meshquadric.so -- quadric placement of the vertices of a vertex clustering (exact int64 quadric sums per cluster, a
                     regularised 3x3 solve in f64) behind include/ngp_meshquadric.h; its sources live under csrc/meshquadric/.
  libngp_meshdecimate.so -- decimation of a mesh to a face budget or an error bound by rounds of independent half-edge collapses
                     (integer plane-distance costs, claim words, the shared compaction) behind include/ngp_meshdecimate.h; its
                     sources live under csrc/meshdecimate/.
  libngp_meshatlas.so -- the texture atlas with texel density by face size (a class per face from its longest edge, a stable
                     16-bucket counting sort, one band of cells per class, texel points, UVs) and its renderer behind
                     csrc/meshatlas/ngp_meshatlas.h, which lies beside its sources under csrc/meshatlas/.
  libngp_meshphoto.so -- the colour of surface points blended from photographs (projection, a two-sided depth test against the
                     mesh's depth buffers, a bilinear sample, a weight by viewing angle, serial per-point sums) behind
                     csrc/meshphoto/ngp_meshphoto.h, which lies beside its sources under csrc/meshphoto/.
  libngp_meshnormal.so -- the normals of a detail mesh carried onto the texels of a simplified one (the nearest face that faces the
                     same way, exactly the brute-force minimum through libngp_meshdist.so's grid; interpolated vertex normals) and
                     the shading of a frame by a rendered normal map behind csrc/meshnormal/ngp_meshnormal.h, which lies beside
                     its sources under csrc/meshnormal/.
  libngp_meshchart.so -- the texture atlas made of charts (snapped integer corners, a class per face from its integer normal,
                     union-find over faces that share an edge, shelves of padded rectangles, texel owners by an atomic minimum,
                     eviction of overlapping faces, dilation, texel points, one UV per vertex and chart) and its renderer behind
                     csrc/meshchart/ngp_meshchart.h, which lies beside its sources under csrc/meshchart/.
  libngp_meshsparse.so -- marching cubes over the 8^3-point bricks of the lattice that touch occupied cells of the occupancy grid
                     (the mask from the bitfield in f64, its dilation, slot lists through the shared scans, the points of the sampled
                     bricks, one workgroup per brick over a sigma tile in LDS) behind csrc/meshsparse/ngp_meshsparse.h, which lies
                     beside its sources under csrc/meshsparse/.  csrc/mesh_mc.h holds the per-point and per-cell rules of marching
                     cubes for this library and libngp_mesh.so, so that both give the same bits.
The mesh libraries share source, each header included inside the including library's anonymous namespace: csrc/mesh_host.h (the
host helpers of the C entry points, every mesh library), csrc/mesh_scan.h (integer sums and prefix sums over a wave, a workgroup
and an array), csrc/mesh_labels.h (the lanes of a wave grouped by label), csrc/mesh_cells.h (the clustering grid of the simplifier
and the quadric placement) and csrc/mesh_mix.h (the 64-bit hash of the tables), beside csrc/mesh_compact.h, csrc/mesh_camera.h,
csrc/mesh_raster.h and csrc/mesh_nearest.h.
Run as `python -m ngp_pl_amd.build` or through `__graft_entry__.build()`.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libngp_hip.so")
SOURCES = ["march.hip", "composite.hip", "hashgrid.hip", "mlp.hip", "optim.hip", "occupancy.hip", "hashgrid_bwd_binned.hip", "stepper.hip", "comm.hip"]
HEADERS = ["ngp_common.h", "hashgrid_common.h", "loss_common.h", "comm.h", "adam_common.h", os.path.join("..", "..", "include", "ngp_hip.h")]
ARCH = "gfx950"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CFLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
          "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-result"]
# per-source extras.  mlp.hip: MFMA results land in VGPRs -- every result of forward/dgrad is consumed by VALU code (convert to
# f16, ReLU), and with the accumulator-register form the compiler chose under this register pressure each of those 16-register
# results cost 16 v_accvgpr_read (208 of the 980 instructions of a backward tile)
EXTRA = {"mlp.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}
MESH_LIB = os.path.join(CSRC, "libngp_mesh.so")
MESH_SOURCES = [os.path.join("mesh", "mesh.hip")]
MESH_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_mc.h", os.path.join("mesh", "mc_tables.h"), os.path.join("..", "..", "include", "ngp_mesh.h")]
# positions and normals are the plain f32 expressions of include/ngp_mesh.h (no fused multiply-add), as tests/mc_reference.py has them
MESH_CFLAGS = ["-ffp-contract=off"]
MESHFILTER_LIB = os.path.join(CSRC, "libngp_meshfilter.so")
MESHFILTER_SOURCES = [os.path.join("meshfilter", "meshfilter.hip")]
MESHFILTER_HEADERS = ["mesh_compact.h", "mesh_host.h", "mesh_scan.h", "mesh_labels.h", os.path.join("..", "..", "include", "ngp_meshfilter.h")]
MESHCULL_LIB = os.path.join(CSRC, "libngp_meshcull.so")
MESHCULL_SOURCES = [os.path.join("meshcull", "meshcull.hip")]
MESHCULL_HEADERS = ["mesh_compact.h", "mesh_host.h", "mesh_scan.h", "mesh_camera.h", "mesh_raster.h", os.path.join("..", "..", "include", "ngp_meshcull.h")]
# projection, edge functions and depths are the plain f32 expressions of include/ngp_meshcull.h, as tests/mesh_visibility_reference.py has them
MESHCULL_CFLAGS = ["-ffp-contract=off"]
MESHSIMPLIFY_LIB = os.path.join(CSRC, "libngp_meshsimplify.so")
MESHSIMPLIFY_SOURCES = [os.path.join("meshsimplify", "meshsimplify.hip")]
MESHSIMPLIFY_HEADERS = ["mesh_compact.h", "mesh_host.h", "mesh_scan.h", "mesh_labels.h", "mesh_cells.h", "mesh_mix.h", os.path.join("..", "..", "include", "ngp_meshsimplify.h")]
# cells, fixed-point fractions and the f64 means are the plain expressions of include/ngp_meshsimplify.h, as tests/mesh_simplify_reference.py has them
MESHSIMPLIFY_CFLAGS = ["-ffp-contract=off"]
MESHTSDF_LIB = os.path.join(CSRC, "libngp_meshtsdf.so")
MESHTSDF_SOURCES = [os.path.join("meshtsdf", "meshtsdf.hip")]
MESHTSDF_HEADERS = ["mesh_host.h", "mesh_camera.h", os.path.join("..", "..", "include", "ngp_meshtsdf.h")]
# lattice points, projection and truncated distances are the plain f32 expressions of include/ngp_meshtsdf.h, as tests/mesh_tsdf_reference.py has them
MESHTSDF_CFLAGS = ["-ffp-contract=off"]
MESHSMOOTH_LIB = os.path.join(CSRC, "libngp_meshsmooth.so")
MESHSMOOTH_SOURCES = [os.path.join("meshsmooth", "meshsmooth.hip")]
MESHSMOOTH_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_mix.h", os.path.join("..", "..", "include", "ngp_meshsmooth.h")]
# grid states, the f64 steps and the normals are the plain expressions of include/ngp_meshsmooth.h, as tests/mesh_smooth_reference.py has them
MESHSMOOTH_CFLAGS = ["-ffp-contract=off"]
MESHTEX_LIB = os.path.join(CSRC, "libngp_meshtex.so")
MESHTEX_SOURCES = [os.path.join("meshtex", "meshtex.hip")]
MESHTEX_HEADERS = ["mesh_host.h", "mesh_camera.h", "mesh_raster.h", os.path.join("..", "..", "include", "ngp_meshtex.h")]
# texel points, directions, projection, barycentric weights and the bilinear lookup are the plain f32 expressions of include/ngp_meshtex.h, as tests/mesh_texture_reference.py has them
MESHTEX_CFLAGS = ["-ffp-contract=off"]
METRICS_LIB = os.path.join(CSRC, "libngp_metrics.so")
METRICS_SOURCES = [os.path.join("metrics", "metrics.hip")]
METRICS_HEADERS = [os.path.join("..", "..", "include", "ngp_metrics.h")]
# the filter taps, the index and the squared error are the plain f32 expressions of include/ngp_metrics.h, as tests/metrics_reference.py has them
METRICS_CFLAGS = ["-ffp-contract=off"]
MESHDIST_LIB = os.path.join(CSRC, "libngp_meshdist.so")
MESHDIST_SOURCES = [os.path.join("meshdist", "meshdist.hip")]
MESHDIST_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_nearest.h", os.path.join("..", "..", "include", "ngp_meshdist.h")]
# samples, the closest point of a triangle and the squared distance are the plain f32 expressions of include/ngp_meshdist.h, as tests/mesh_distance_reference.py has them
MESHDIST_CFLAGS = ["-ffp-contract=off"]
MESHQUADRIC_LIB = os.path.join(CSRC, "libngp_meshquadric.so")
MESHQUADRIC_SOURCES = [os.path.join("meshquadric", "meshquadric.hip")]
MESHQUADRIC_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_labels.h", "mesh_cells.h", os.path.join("..", "..", "include", "ngp_meshquadric.h")]
# cells, planes, weights, the rounding to int64 and the f64 solve are the plain expressions of include/ngp_meshquadric.h, as tests/mesh_quadric_reference.py has them
MESHQUADRIC_CFLAGS = ["-ffp-contract=off"]
MESHDECIMATE_LIB = os.path.join(CSRC, "libngp_meshdecimate.so")
MESHDECIMATE_SOURCES = [os.path.join("meshdecimate", "meshdecimate.hip")]
MESHDECIMATE_HEADERS = ["mesh_compact.h", "mesh_host.h", "mesh_scan.h", os.path.join("..", "..", "include", "ngp_meshdecimate.h")]
# cross products, the flip and error tests and the rounding of the costs to int64 are the plain f64 expressions of include/ngp_meshdecimate.h, as tests/mesh_decimate_reference.py has them
MESHDECIMATE_CFLAGS = ["-ffp-contract=off"]
MESHATLAS_LIB = os.path.join(CSRC, "libngp_meshatlas.so")
MESHATLAS_SOURCES = [os.path.join("meshatlas", "meshatlas.hip")]
MESHATLAS_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_camera.h", "mesh_raster.h", os.path.join("meshatlas", "ngp_meshatlas.h")]
# edge lengths, class thresholds, texel points, projection, barycentric weights and the bilinear lookup are the plain f32 expressions of csrc/meshatlas/ngp_meshatlas.h, as tests/mesh_atlas_reference.py has them
MESHATLAS_CFLAGS = ["-ffp-contract=off"]
MESHPHOTO_LIB = os.path.join(CSRC, "libngp_meshphoto.so")
MESHPHOTO_SOURCES = [os.path.join("meshphoto", "meshphoto.hip")]
MESHPHOTO_HEADERS = ["mesh_host.h", "mesh_camera.h", os.path.join("meshphoto", "ngp_meshphoto.h")]
# projection, the viewing angle, the depth test, the bilinear sample and the weighted sums are the plain f32 expressions of csrc/meshphoto/ngp_meshphoto.h, as tests/mesh_photo_reference.py has them
MESHPHOTO_CFLAGS = ["-ffp-contract=off"]
MESHNORMAL_LIB = os.path.join(CSRC, "libngp_meshnormal.so")
MESHNORMAL_SOURCES = [os.path.join("meshnormal", "meshnormal.hip")]
MESHNORMAL_HEADERS = ["mesh_host.h", "mesh_nearest.h", os.path.join("meshnormal", "ngp_meshnormal.h")]
# the orientation test, the closest point of a triangle, the interpolated normal and the shading are the plain f32 expressions of csrc/meshnormal/ngp_meshnormal.h, as tests/mesh_normal_reference.py has them
MESHNORMAL_CFLAGS = ["-ffp-contract=off"]
MESHCHART_LIB = os.path.join(CSRC, "libngp_meshchart.so")
MESHCHART_SOURCES = [os.path.join("meshchart", "meshchart.hip")]
MESHCHART_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_camera.h", "mesh_raster.h", os.path.join("meshchart", "ngp_meshchart.h")]
# the snap, the f64 quotients, texel points, projection, barycentric weights and the bilinear lookup are the plain expressions of csrc/meshchart/ngp_meshchart.h, as tests/mesh_chart_reference.py has them
MESHCHART_CFLAGS = ["-ffp-contract=off"]
MESHSPARSE_LIB = os.path.join(CSRC, "libngp_meshsparse.so")
MESHSPARSE_SOURCES = [os.path.join("meshsparse", "meshsparse.hip")]
MESHSPARSE_HEADERS = ["mesh_host.h", "mesh_scan.h", "mesh_mc.h", os.path.join("mesh", "mc_tables.h"), os.path.join("meshsparse", "ngp_meshsparse.h")]
# positions, edge parameters and normals are the plain f32 expressions of include/ngp_mesh.h and the occupancy rule the plain f64 expressions of csrc/meshsparse/ngp_meshsparse.h, as tests/mesh_sparse_reference.py has them
MESHSPARSE_CFLAGS = ["-ffp-contract=off"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed: %s\n%s" % (" ".join(cmd), r.stdout))
    return r.stdout


def _plan(sources, headers, extra, force):
    hdrs = [os.path.join(CSRC, h) for h in headers]
    objs, jobs = [], []
    for src in sources:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s, os.path.abspath(__file__)] + hdrs):
            jobs.append([HIPCC] + CFLAGS + extra(src) + ["-c", s, "-o", o])
    return objs, jobs


def build(force=False, verbose=False):
    objs, jobs = _plan(SOURCES, HEADERS, lambda src: EXTRA.get(src, []), force)
    mesh_objs, mesh_jobs = _plan(MESH_SOURCES, MESH_HEADERS, lambda src: MESH_CFLAGS, force)
    filter_objs, filter_jobs = _plan(MESHFILTER_SOURCES, MESHFILTER_HEADERS, lambda src: [], force)
    cull_objs, cull_jobs = _plan(MESHCULL_SOURCES, MESHCULL_HEADERS, lambda src: MESHCULL_CFLAGS, force)
    simplify_objs, simplify_jobs = _plan(MESHSIMPLIFY_SOURCES, MESHSIMPLIFY_HEADERS, lambda src: MESHSIMPLIFY_CFLAGS, force)
    tsdf_objs, tsdf_jobs = _plan(MESHTSDF_SOURCES, MESHTSDF_HEADERS, lambda src: MESHTSDF_CFLAGS, force)
    smooth_objs, smooth_jobs = _plan(MESHSMOOTH_SOURCES, MESHSMOOTH_HEADERS, lambda src: MESHSMOOTH_CFLAGS, force)
    tex_objs, tex_jobs = _plan(MESHTEX_SOURCES, MESHTEX_HEADERS, lambda src: MESHTEX_CFLAGS, force)
    metrics_objs, metrics_jobs = _plan(METRICS_SOURCES, METRICS_HEADERS, lambda src: METRICS_CFLAGS, force)
    dist_objs, dist_jobs = _plan(MESHDIST_SOURCES, MESHDIST_HEADERS, lambda src: MESHDIST_CFLAGS, force)
    quadric_objs, quadric_jobs = _plan(MESHQUADRIC_SOURCES, MESHQUADRIC_HEADERS, lambda src: MESHQUADRIC_CFLAGS, force)
    decimate_objs, decimate_jobs = _plan(MESHDECIMATE_SOURCES, MESHDECIMATE_HEADERS, lambda src: MESHDECIMATE_CFLAGS, force)
    atlas_objs, atlas_jobs = _plan(MESHATLAS_SOURCES, MESHATLAS_HEADERS, lambda src: MESHATLAS_CFLAGS, force)
    photo_objs, photo_jobs = _plan(MESHPHOTO_SOURCES, MESHPHOTO_HEADERS, lambda src: MESHPHOTO_CFLAGS, force)
    normal_objs, normal_jobs = _plan(MESHNORMAL_SOURCES, MESHNORMAL_HEADERS, lambda src: MESHNORMAL_CFLAGS, force)
    chart_objs, chart_jobs = _plan(MESHCHART_SOURCES, MESHCHART_HEADERS, lambda src: MESHCHART_CFLAGS, force)
    sparse_objs, sparse_jobs = _plan(MESHSPARSE_SOURCES, MESHSPARSE_HEADERS, lambda src: MESHSPARSE_CFLAGS, force)
    todo = (jobs + mesh_jobs + filter_jobs + cull_jobs + simplify_jobs + tsdf_jobs + smooth_jobs + tex_jobs + metrics_jobs + dist_jobs
            + quadric_jobs + decimate_jobs + atlas_jobs + photo_jobs + normal_jobs + chart_jobs + sparse_jobs)
    if todo:
        if verbose:
            print("[ngp_pl_amd.build] compiling %d HIP sources for %s" % (len(todo), ARCH))
        with ThreadPoolExecutor(max_workers=min(len(todo), os.cpu_count() or 1)) as ex:
            list(ex.map(_run, todo))
    for lib, o, changed in ((LIB, objs, jobs), (MESH_LIB, mesh_objs, mesh_jobs), (MESHFILTER_LIB, filter_objs, filter_jobs),
                            (MESHCULL_LIB, cull_objs, cull_jobs), (MESHSIMPLIFY_LIB, simplify_objs, simplify_jobs),
                            (MESHTSDF_LIB, tsdf_objs, tsdf_jobs), (MESHSMOOTH_LIB, smooth_objs, smooth_jobs),
                            (MESHTEX_LIB, tex_objs, tex_jobs), (METRICS_LIB, metrics_objs, metrics_jobs),
                            (MESHDIST_LIB, dist_objs, dist_jobs), (MESHQUADRIC_LIB, quadric_objs, quadric_jobs),
                            (MESHDECIMATE_LIB, decimate_objs, decimate_jobs), (MESHATLAS_LIB, atlas_objs, atlas_jobs),
                            (MESHPHOTO_LIB, photo_objs, photo_jobs), (MESHNORMAL_LIB, normal_objs, normal_jobs),
                            (MESHCHART_LIB, chart_objs, chart_jobs), (MESHSPARSE_LIB, sparse_objs, sparse_jobs)):
        if force or changed or _stale(lib, o):
            _run([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC"] + o + ["-o", lib])
            if verbose:
                print("[ngp_pl_amd.build] linked", lib)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
