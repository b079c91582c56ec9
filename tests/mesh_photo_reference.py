"""Plain numpy float32 restatement of libngp_meshphoto.so (ngp_pl_amd/csrc/meshphoto/ngp_meshphoto.h, THE RULE), expression for
expression: every product and sum below is one f32 operation in the header's order (no `@`, no fused multiply-add), divisions and
square roots are numpy's correctly rounded f32 ones.  `accumulate`, `resolve`, `photo_colors`; the hand-worked cases and the
scenes the CPU and GPU tests share (a random plane scene, a fronto-parallel square with an affine colour, two parallel squares).
Test infrastructure only."""
import numpy as np

from tests import mesh_texture_reference as TR
from tests import mesh_visibility_reference as MV

F = np.float32
INF_BITS = 0x7F800000
CAM_TILE = 64                                           # cameras per LDS tile of the kernel; the tests straddle it


def accumulate(points, dirs, valid, K, poses, img_wh, images, zbuf, near, bias, guard, min_cos, power, acc=None, views=None):
    """acc (n, 4) f32 and views (n,) i32 after the cameras of `poses`, in ascending order, on top of the given acc and views (zeros
    by default; the inputs are not modified)."""
    W, H = int(img_wh[0]), int(img_wh[1])
    x = np.asarray(points, F).reshape(-1, 3)
    g = np.asarray(dirs, F).reshape(-1, 3)
    n = len(x)
    K = np.asarray(K, F)
    poses = np.asarray(poses, F)[:, :3, :4]
    images = np.asarray(images, np.uint8).reshape(len(poses), H, W, 3)
    zbuf = np.ascontiguousarray(np.asarray(zbuf).reshape(len(poses), H, W)).view(np.uint32).view(F)
    acc = np.zeros((n, 4), F) if acc is None else np.array(acc, F).reshape(n, 4)
    views = np.zeros(n, np.int32) if views is None else np.array(views, np.int32).reshape(n)
    near, bias, min_cos, guard, power = F(near), F(bias), F(min_cos), int(guard), int(power)
    if not (0 <= guard <= 4 and 1 <= power <= 8 and 0 < min_cos <= 1 and bias >= 0 and np.isfinite(bias) and np.isfinite(near)):
        raise ValueError("argument out of range")
    with np.errstate(all="ignore"):
        live = (np.asarray(valid).reshape(n) != 0) & np.isfinite(x).all(1) & np.isfinite(g).all(1)
        u_max, v_max = F(W) - F(0.5), F(H) - F(0.5)
        for c in range(len(poses)):
            m, s = MV.camera_rows(poses[c])
            o = poses[c][:, 3]
            p = [m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1] + m[r, 2] * x[:, 2] + s[r] for r in range(3)]
            ud, vd, d = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
            u, v = ud / d, vd / d
            ok = live & (d >= near)                                                     # 1
            ok &= (u >= F(0.5)) & (u <= u_max) & (v >= F(0.5)) & (v <= v_max)           # 2
            e0, e1, e2 = o[0] - x[:, 0], o[1] - x[:, 1], o[2] - x[:, 2]
            L = np.sqrt((e0 * e0 + e1 * e1) + e2 * e2)
            cs = -((g[:, 0] * e0 + g[:, 1] * e1) + g[:, 2] * e2) / L
            ok &= (L > 0) & (cs >= min_cos)                                             # 3
            k = np.nonzero(ok)[0]                       # every index below comes from a u, v that passed test 2
            if not len(k):
                continue
            uk, vk, dk = u[k], v[k], d[k]
            ic, jc = np.floor(uk).astype(np.int64), np.floor(vk).astype(np.int64)
            agree = np.ones(len(k), bool)
            for dj in range(-guard, guard + 1):                                         # 4
                for di in range(-guard, guard + 1):
                    i, j = ic + di, jc + dj
                    inside = (i >= 0) & (i <= W - 1) & (j >= 0) & (j <= H - 1)
                    z = zbuf[c][np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)]
                    agree &= ~inside | ((dk <= z + bias) & (z <= dk + bias))
            k, uk, vk = k[agree], uk[agree], vk[agree]
            if not len(k):
                continue
            X, Y = uk - F(0.5), vk - F(0.5)
            i0, j0 = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
            fx, fy = X - np.floor(X), Y - np.floor(Y)
            i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
            w = cs[k]
            for _ in range(power - 1):
                w = w * cs[k]
            img = images[c]
            for ch in range(3):
                t = lambda i, j: img[j, i, ch].astype(F)
                top = t(i0, j0) * (F(1) - fx) + t(i1, j0) * fx
                bot = t(i0, j1) * (F(1) - fx) + t(i1, j1) * fx
                col = top * (F(1) - fy) + bot * fy
                acc[k, ch] = acc[k, ch] + w * col
            acc[k, 3] = acc[k, 3] + w
            views[k] += 1
    return acc, views


def resolve(acc, views, valid, min_views):
    """rgb (n, 3) f32 and seen (n,) u8."""
    acc = np.asarray(acc, F).reshape(-1, 4)
    if int(min_views) < 1:
        raise ValueError("min_views >= 1")
    seen = (np.asarray(valid).reshape(-1) != 0) & (np.asarray(views).reshape(-1) >= int(min_views)) & (acc[:, 3] > 0)
    rgb = np.zeros((len(acc), 3), F)
    with np.errstate(all="ignore"):
        for ch in range(3):
            rgb[seen, ch] = (acc[seen, ch] / acc[seen, 3]) / F(255)
    return rgb, seen.astype(np.uint8)


def depth_buffers(vertices, faces, K, poses, img_wh, near):
    """(C, H, W) u32 depth bits of the mesh, the rule of include/ngp_meshcull.h."""
    return MV.zbuffers(vertices, faces, K, poses, img_wh, near)


def photo_colors(vertices, faces, points, dirs, valid, images, K, poses, img_wh, bias, guard=1, min_cos=0.1, power=2, min_views=1, near=0.01,
                 zbuf=None):
    """rgb, seen, views as ngp_pl_amd.mesh.photo_colors returns them."""
    if zbuf is None:
        zbuf = depth_buffers(vertices, faces, K, poses, img_wh, near)
    acc, views = accumulate(points, dirs, valid, K, poses, img_wh, images, zbuf, near, bias, guard, min_cos, power)
    rgb, seen = resolve(acc, views, valid, min_views)
    return rgb, seen, views


def quantise(rgb):
    """round(clamp(c, 0, 1) * 255) as u8, halves to even: mesh._quantise."""
    return np.rint(np.clip(np.asarray(rgb, F), F(0), F(1)) * F(255)).astype(np.uint8)


def words(a):
    """The int32 words of an f32 array: what the bit-for-bit comparisons compare."""
    return np.ascontiguousarray(np.asarray(a, F)).view(np.int32)


# ---- hand-worked cases: one point, one camera at the origin looking along +z, a 4 x 4 photograph -----------------------------

IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(F)


def hand_image():
    """(1, 4, 4, 3) u8 with byte 10 i + 40 j + k at pixel (i, j), channel k."""
    j, i, k = np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij")
    return (10 * i + 40 * j + k).astype(np.uint8)[None]


def _ones_zbuf(holes=(), depth=1.0):
    z = np.full((1, 4, 4), F(depth), F)
    for i, j in holes:
        z[0, j, i] = np.inf
    return z.view(np.uint32)


def _hand(name, accepted, point, cx=0.0, dir=(0, 0, 1), zbuf=None, near=0.5, bias=0.0, guard=1, min_cos=0.1, power=2, col=None):
    K = np.array([[1, 0, cx], [0, 1, cx], [0, 0, 1]], F)
    return dict(name=name, accepted=accepted, points=np.array([point], F), dirs=np.array([dir], F), valid=np.ones(1, np.uint8), K=K,
                poses=IDENTITY[None], img_wh=(4, 4), images=hand_image(), zbuf=_ones_zbuf() if zbuf is None else zbuf, near=near, bias=bias,
                guard=guard, min_cos=min_cos, power=power, col=col)


def hand_cases():
    """The boundary cases of THE RULE.  The camera sits at the origin with R = I, so p = x and d = x2.  With cx = 0 a point
    (a, b, 1) has u = a and v = b exactly; with cx = 2 a point (0, 0, d) has u = v = 2 d / d = 2 exactly, whatever d.  `accepted`
    says whether the one sample is taken; `col`, where given, is the colour (3,) that the bilinear read must give, worked by hand:
    byte(i, j, k) = 10 i + 40 j + k."""
    up, down = (lambda a: np.nextafter(F(a), F(np.inf))), (lambda a: np.nextafter(F(a), F(-np.inf)))
    one_up = up(1.0)
    cases = [
        # u = 2.5 is the centre of pixel 2: X = 2, fx = 0; v = 1.25: Y = 0.75, j0 = 0, fy = 0.75:
        # col = byte(2, 0) * 0.25 + byte(2, 1) * 0.75 = (20 + k) / 4 + 3 (60 + k) / 4 = 50 + k
        _hand("pixel centre, fx == 0", True, (2.5, 1.25, 1), col=(50, 51, 52)),
        # u = 2, v = 3: X = 1.5, Y = 2.5: the mean of the bytes of pixels (1..2, 2..3) = 10 * 1.5 + 40 * 2.5 + k
        _hand("between four pixels", True, (2, 3, 1), col=(115, 116, 117)),
        # u = 0.5: X = 0, i0 = 0, fx = 0; v = 0.5 likewise: byte(0, 0)
        _hand("u == 0.5 and v == 0.5", True, (0.5, 0.5, 1), col=(0, 1, 2)),
        _hand("u one ulp below 0.5", False, (down(0.5), 0.5, 1)),
        _hand("v one ulp below 0.5", False, (0.5, down(0.5), 1)),
        # u = 3.5: X = 3, i0 = 3, i1 = min(4, 3) = 3, fx = 0: byte(3, 3)
        _hand("u == W - 0.5 and v == H - 0.5", True, (3.5, 3.5, 1), col=(150, 151, 152)),
        _hand("u one ulp above W - 0.5", False, (up(3.5), 3.5, 1)),
        _hand("v one ulp above H - 0.5", False, (3.5, up(3.5), 1)),
        # d == near
        _hand("d == near", True, (0, 0, 1), cx=2.0, near=1.0),
        _hand("d one ulp below near", False, (0, 0, 1), cx=2.0, near=one_up),
        # d == z + bias: z = 0.75, bias = 0.25; the next d up fails the first half of test 4 (z + bias = 1 < d)
        _hand("d == z + bias", True, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(depth=0.75), bias=0.25),
        _hand("d one ulp above z + bias", False, (0, 0, one_up), cx=2.0, zbuf=_ones_zbuf(depth=0.75), bias=0.25),
        # the other side: z == d + bias with z = 1.25, and the next z up
        _hand("z == d + bias", True, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(depth=1.25), bias=0.25),
        _hand("z one ulp above d + bias", False, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(depth=up(1.25)), bias=0.25),
        # on the axis e = (0, 0, -1), L = 1 and cs = dir2
        _hand("cs == min_cos", True, (0, 0, 1), cx=2.0, dir=(0.5, -0.5, 0.25), min_cos=0.25),
        _hand("cs one ulp below min_cos", False, (0, 0, 1), cx=2.0, dir=(0.5, -0.5, 0.25), min_cos=up(0.25)),
        _hand("facing away", False, (0, 0, 1), cx=2.0, dir=(0, 0, -1)),
        # an empty pixel inside the window rejects; outside it does not
        _hand("empty pixel in the window", False, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(holes=[(3, 1)])),
        _hand("empty pixel outside the window (guard 0)", True, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(holes=[(3, 1)]), guard=0),
        _hand("empty centre pixel", False, (0, 0, 1), cx=2.0, zbuf=_ones_zbuf(holes=[(2, 2)]), guard=0),
        # pixel (0, 0) with guard 4: the window is clipped to the whole 4 x 4 image, pixel (3, 3) is in it from guard 3 on
        _hand("window clipped at the corner, all agree", True, (0.5, 0.5, 1), guard=4, col=(0, 1, 2)),
        _hand("window clipped at the corner, far pixel empty, guard 4", False, (0.5, 0.5, 1), zbuf=_ones_zbuf(holes=[(3, 3)]), guard=4),
        _hand("window clipped at the corner, far pixel empty, guard 3", False, (0.5, 0.5, 1), zbuf=_ones_zbuf(holes=[(3, 3)]), guard=3),
        _hand("window clipped at the corner, far pixel empty, guard 2", True, (0.5, 0.5, 1), zbuf=_ones_zbuf(holes=[(3, 3)]), guard=2, col=(0, 1, 2)),
        _hand("window clipped at the far corner", False, (3.5, 3.5, 1), zbuf=_ones_zbuf(holes=[(0, 3)]), guard=4),
        # power: w = cs, cs * cs, ... on the axis with cs = 0.5
        _hand("power 1", True, (0, 0, 1), cx=2.0, dir=(0, 0, 0.5), power=1),
        _hand("power 8", True, (0, 0, 1), cx=2.0, dir=(0, 0, 0.5), power=8),
    ]
    return cases


def run_case(case, fn=accumulate):
    return fn(case["points"], case["dirs"], case["valid"], case["K"], case["poses"], case["img_wh"], case["images"], case["zbuf"],
              case["near"], case["bias"], case["guard"], case["min_cos"], case["power"])


# ---- a random scene: points scattered about the plane z = 0 that a square mesh covers ----------------------------------------

SQUARE_V = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
SQUARE_F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def cameras_above(n_cams, img_wh, seed, spread=0.5, height=(2.0, 3.0), fill=0.9):
    """K and n_cams poses above the plane z = 0, looking down at points near the origin."""
    g = np.random.RandomState(seed)
    W, H = img_wh
    focal = fill * min(W, H) * height[0] / 2.0           # the square of side 2 about fills the smaller side from the lowest camera
    K = MV.intrinsics(focal, W / 2.0, H / 2.0)
    poses = []
    for _ in range(n_cams):
        eye = np.array([g.uniform(-spread, spread), g.uniform(-spread, spread), g.uniform(*height)])
        target = np.array([g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2), 0.0])
        poses.append(MV.look_at(eye, target, up=(0.0, 1.0, 0.0)))
    return K, np.stack(poses)


def random_scene(n, img_wh, n_cams, seed, bias=0.25, extent=1.0):
    """n points within about a bias of the plane (some in front, some behind, some past the square's edge), directions about
    (0, 0, -1) (the viewer looks down), random valid flags and random photographs; the depth buffers are those of the square,
    scaled by `extent` (3: it fills every photograph, no pixel is empty)."""
    g = np.random.RandomState(seed)
    K, poses = cameras_above(n_cams, img_wh, seed + 1)
    W, H = img_wh
    points = np.stack([g.uniform(-1.2, 1.2, n), g.uniform(-1.2, 1.2, n), g.normal(0, 0.6 * bias, n)], 1).astype(F)
    dirs = np.stack([g.normal(0, 0.5, n), g.normal(0, 0.5, n), -np.ones(n)], 1)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
    dirs[g.rand(n) < 0.1] *= F(-1)                                                      # some face away
    valid = (g.rand(n) < 0.85).astype(np.uint8)
    images = g.randint(0, 256, (n_cams, H, W, 3)).astype(np.uint8)
    zbuf = depth_buffers(F(extent) * SQUARE_V, SQUARE_F, K, poses, img_wh, 0.01)
    return dict(points=points, dirs=dirs, valid=valid, K=K, poses=poses, img_wh=img_wh, images=images, zbuf=zbuf, near=0.01, bias=bias, guard=1,
                min_cos=0.1, power=2)


# ---- a fronto-parallel square with a colour affine in position ----------------------------------------------------------------

LIN_G = np.array([[0.20, 0.10], [-0.15, 0.20], [0.10, -0.25]])                          # |G x| <= 0.35 on the square


def lin(points):
    """(n, 3) f64 in [0.15, 0.85]: 0.5 + G (x0, x1)."""
    p = np.asarray(points, np.float64)
    return 0.5 + p[:, :2] @ LIN_G.T


def fronto_cameras():
    """Cameras that share one rotation (looking straight down at the plane z = 0) and differ in offset and distance."""
    eyes = [(0.0, 0.0, 2.5), (0.3, -0.2, 3.0), (-0.25, 0.15, 2.0), (0.1, 0.3, 3.5)]
    R = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float64)                       # right = +x, down = -y, forward = -z
    return np.stack([np.concatenate([R, np.asarray(e, np.float64)[:, None]], 1) for e in eyes]).astype(F)


def fronto_scene(img_wh=(40, 32), focal=24.0):
    """K, poses, photographs whose bytes are round(255 lin(the point of the plane under the pixel's centre)), and the square's depth
    buffers."""
    W, H = img_wh
    K = MV.intrinsics(focal, W / 2.0, H / 2.0)
    poses = fronto_cameras()
    i, j = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    images = []
    for P in poses.astype(np.float64):
        h = P[2, 3]                                      # the plane lies h in front of the camera
        x = P[0, 3] + (i - W / 2.0) / focal * h
        y = P[1, 3] - (j - H / 2.0) / focal * h
        images.append(np.rint(255.0 * lin(np.stack([x.ravel(), y.ravel()], 1))).reshape(H, W, 3))
    images = np.clip(np.stack(images), 0, 255).astype(np.uint8)
    return K, poses, images, depth_buffers(SQUARE_V, SQUARE_F, K, poses, img_wh, 0.01)


# ---- two parallel squares of different constant colours -------------------------------------------------------------------------

GAP = 1.0
REAR_RGB, FRONT_RGB, BACK_RGB = (40, 200, 90), (220, 30, 60), (255, 255, 255)
TWO_V = np.concatenate([SQUARE_V, np.array([[-0.5, -0.5, GAP], [0.5, -0.5, GAP], [0.5, 0.5, GAP], [-0.5, 0.5, GAP]], F)])
TWO_F = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
TWO_N = np.tile(np.array([[0, 0, 1]], F), (8, 1))
TWO_BOX = ((-2, -2, -2), (2, 2, 2))
TWO_TEXELS = 24                                         # texel intervals per face leg of the atlas the tests bake
TWO_BIAS = 0.1                                          # GAP is ten times this


def two_squares_scene(img_wh=(64, 48), focal=56.0):
    """K, poses (one camera head-on, two oblique), photographs (C, H, W, 3) u8 and depth buffers (C, H, W) u32 of the two squares.
    Both come from ONE raster, the key buffer of tests/mesh_texture_reference.py (the coverage rule of include/ngp_meshcull.h: the
    nearest face per pixel centre): the depth is the key's upper word, and the pixel has the colour of the key's face.  face
    (C, H, W) i32 is that face, -1 for none."""
    W, H = img_wh
    K = MV.intrinsics(focal, W / 2.0, H / 2.0)
    poses = np.stack([MV.look_at(e, (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)) for e in ((0.0, 0.0, 3.5), (0.8, 0.2, 3.3), (-0.5, -0.7, 3.4))])
    keys = TR.key_buffers(TWO_V, TWO_F, K, poses, img_wh, 0.01)
    zbuf = (keys >> np.uint64(32)).astype(np.uint32)
    face = np.where(keys == TR.NO_KEY, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    zbuf[face < 0] = INF_BITS
    palette = np.array([REAR_RGB, REAR_RGB, FRONT_RGB, FRONT_RGB, BACK_RGB], np.uint8)
    images = palette[face]                               # -1 picks the background
    return K, poses, images, zbuf, face


def centre_pixel_face(points, K, poses, img_wh, face, near=0.01):
    """(C, n) i32: the face the raster put at the pixel that holds each point's projection; -2 where the point is outside the
    frame or nearer than `near`."""
    W, H = img_wh
    out = np.full((len(poses), len(points)), -2, np.int32)
    with np.errstate(all="ignore"):
        for c, P in enumerate(np.asarray(poses, F)):
            u, v, d = MV.project(points, K, P)
            inside = (d >= F(near)) & (u >= 0) & (u < F(W)) & (v >= 0) & (v < F(H))
            i, j = np.floor(u[inside]).astype(np.int64), np.floor(v[inside]).astype(np.int64)
            out[c, inside] = face[c][j, i]
    return out
