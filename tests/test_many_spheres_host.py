"""The binned sphere path's host side (CPU): rtm_bin_plan -- the code the render path
sizes and fills its per-tile sphere lists from -- checked against the oracle's own
rasterizer, its treatment of spheres that cover nothing, validation without a device,
and one golden hash that pins scenes.sphere_field and the oracle on this platform."""
import ctypes as C
import dataclasses
import hashlib
import json
import math
import os

import numpy as np
import pytest

W, H = 200, 136
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_spheres.json")


def _covered(oracle, scenes, sphere, cam, w=W, h=H):
    """Pixels the oracle's rasterizer covers with `sphere` alone (either face)."""
    one = scenes.Scene([scenes.PrimitiveSphere(0, sphere.shading, sphere.pos, sphere.r)], [])
    m = np.zeros((h, w), bool)
    for face in (scenes.EnumFace.FRONT, scenes.EnumFace.BACK):
        vp = oracle.Viewport(w, h, face, cam)
        vp.rasterize(one)
        m |= np.isfinite(vp.zbuffer())
    return m


def _cover_counts(oracle, scenes, scene, cam, tw, th, shape, w=W, h=H):
    """Per tile: the spheres covering a pixel of it, and the spheres whose covered
    bounding box, grown by one tile on every side, reaches it."""
    cover = np.zeros(shape, np.int64)
    box = np.zeros(shape, np.int64)
    for s in scene.spherePrimitives:
        ys, xs = np.nonzero(_covered(oracle, scenes, s, cam, w, h))
        if len(ys) == 0:
            continue
        for ty, tx in set(zip((ys // th).tolist(), (xs // tw).tolist())):
            cover[ty, tx] += 1
        box[max(ys.min() // th - 1, 0):ys.max() // th + 2, max(xs.min() // tw - 1, 0):xs.max() // tw + 2] += 1
    return cover, box


def moved_eye(scenes):
    """eye_camera() translated off the axes (the rays keep their direction)."""
    return dataclasses.replace(scenes.eye_camera(), position=(-1.0, 0.13, -0.21))


def _camera(scenes, cam):
    return {"eye": scenes.eye_camera, "shadow": scenes.shadow_camera, "tilted": scenes.tilted_shadow_camera,
            "moved": lambda: moved_eye(scenes)}[cam]()


# (the first two keep the ids they had before the other cameras and sizes joined them)
_PLAN_CASES = [pytest.param("eye", W, H, id="eye"), pytest.param("shadow", W, H, id="shadow")]
_PLAN_CASES += [pytest.param(c, w, h, id=f"{c}-{w}x{h}") for w, h in ((W, H), (65, 9), (4097, 3))
                for c in ("eye", "shadow", "tilted", "moved") if (w, h) != (W, H) or c in ("tilted", "moved")]


@pytest.mark.parametrize("cam,w,h", _PLAN_CASES)
def test_bin_plan_is_conservative_and_culls(rtm, scenes, oracle, cam, w, h):
    camera = _camera(scenes, cam)
    old = (w, h) == (W, H) and cam in ("eye", "shadow")
    scene = scenes.sphere_field(300 if old else 120)
    (tw, th), counts = rtm.bin_plan(scene, camera, w, h)
    assert counts.shape == (-(-h // th), -(-w // tw))
    cover, box = _cover_counts(oracle, scenes, scene, camera, tw, th, counts.shape, w, h)
    assert cover.sum() > 0
    assert (counts >= cover).all(), "a tile's list misses a sphere that covers a pixel of it"
    if old:
        # the cull must bite: the bound holds for the reference's own bounding boxes plus a
        # tile of margin (checked here, so the bound is not one only the plan could meet)
        bound = len(scene.spherePrimitives) * counts.size / 4
        assert box.sum() < bound
        assert counts.sum() < bound
    assert counts.sum() <= box.sum()


def test_single_spheres_of_every_scale_are_in_their_tiles(rtm, scenes, oracle):
    """A seeded loop of one-sphere scenes, |r| from 1e-4 to 3 and either sign, centres at
    random, on pixel sample points and on tile corners (a sphere far smaller than a pixel
    covers the one pixel whose sample point it sits on): every pixel the oracle covers
    lies in a tile whose count is 1."""
    u = scenes.splitmix64(0x51)
    S = scenes.Shading(1.0, 1.0, 1.0)
    covering = tiny_covering = 0
    for case in range(30):
        cam_name = ("eye", "shadow")[case % 2]
        cam = _camera(scenes, cam_name)
        r = 10.0 ** (-4.0 + (math.log10(3.0) + 4.0) * next(u)) * (-1.0 if next(u) < 0.5 else 1.0)
        kind = case % 3
        if kind == 0:
            sx, sy = -0.95 + 1.9 * next(u), -0.95 + 1.9 * next(u)
        else:  # the NDC of pixel (i, j)'s sample point, (i / W) * 2 - 1; kind 2: a tile's first pixel
            i, j = int(next(u) * W), int(next(u) * H)
            if kind == 2:
                i, j = i // 64 * 64, j // 8 * 8
            sx, sy = (i / W) * 2.0 - 1.0, (j / H) * 2.0 - 1.0
        depth = 0.5 * next(u)
        # screen (x, y) is world (z, y) for the eye and world (x, y) for the sun
        pos = (depth, sy, sx) if cam_name == "eye" else (sx, sy, 0.5 + depth)
        sphere = scenes.PrimitiveSphere(0, S, pos, r)
        covered = _covered(oracle, scenes, sphere, cam)
        (tw, th), counts = rtm.bin_plan(scenes.Scene([sphere], []), cam, W, H)
        assert counts.max() <= 1, (case, pos, r)
        ys, xs = np.nonzero(covered)
        assert (counts[ys // th, xs // tw] == 1).all(), (case, pos, r)
        covering += len(ys) > 0
        tiny_covering += len(ys) > 0 and abs(r) < 0.005  # (half a pixel is 0.005 wide)
    assert covering >= 20 and tiny_covering >= 3


def stack(scenes, n, r):
    """n spheres, each a little nearer to both cameras than the one before: the last in
    scene order is the nearest wherever it covers (tests/test_many_spheres_edges.py)."""
    return scenes.Scene([scenes.PrimitiveSphere(i, scenes.Shading(*scenes._COLORS_B[i % 4]),
                                                (-1e-3 * i, 0.0, -1e-3 * i), r) for i in range(n)],
                        [scenes.BENCH_PATCH])


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_chunk_seam_stacks_have_n_entries_everywhere(rtm, scenes, n):
    for cam in (scenes.eye_camera(), scenes.shadow_camera()):
        counts = rtm.bin_plan(stack(scenes, n, 5.0), cam, W, H)[1]
        assert counts.shape == (17, 4) and counts.min() == counts.max() == n


def refusal_scene(scenes):
    """65536 spheres over the whole image: at 7680x4320 every one of 64800 tile lists holds
    them all, more than 2^31-1 entries per viewport."""
    white = scenes.Shading(1.0, 1.0, 1.0)
    return scenes.Scene([scenes.PrimitiveSphere(i, white, (0.0, 0.0, 0.0), 5.0) for i in range(65536)],
                        [scenes.BENCH_PATCH])


def test_plan_past_int32_sums_without_wrap(rtm, scenes):
    counts = rtm.bin_plan(refusal_scene(scenes), scenes.eye_camera(), 7680, 4320)[1]
    assert counts.shape == (540, 120) and counts.dtype == np.int32
    assert (counts == 65536).all()
    assert int(counts.astype(np.int64).sum()) == 64800 * 65536 > 2 ** 31 - 1


def test_spheres_that_cover_nothing_are_in_no_list(rtm, scenes, oracle):
    S = scenes.Shading(1.0, 1.0, 1.0)
    eye = scenes.eye_camera()

    def plan(pos, r):
        return rtm.bin_plan(scenes.Scene([scenes.PrimitiveSphere(0, S, pos, r)], []), eye, W, H)[1]

    assert plan((0.0, 0.0, 0.5), 0.0).sum() == 0
    assert plan((0.0, math.nan, 0.5), 0.3).sum() == 0
    assert plan((0.0, 0.0, 0.5), math.nan).sum() == 0
    assert plan((0.0, 0.0, 0.5), math.inf).sum() == 0
    assert plan((0.0, 50.0, 0.5), 0.3).sum() == 0       # far above the image
    assert plan((0.0, 0.0, -40.0), 0.3).sum() == 0      # far left of it (screen x is world z)
    # a sphere over the whole image is in every tile's list once
    assert (plan((0.0, 0.0, 0.0), 5.0) == 1).all()
    # A negative radius is not such a sphere: the reference covers pixels with it (the
    # ellipse test squares the sign away, main.rs:2848-2852), so does the oracle, and the
    # plan must hold it wherever it does.
    neg = scenes.PrimitiveSphere(0, S, (0.0, 0.0, 0.5), -0.3)
    covered = _covered(oracle, scenes, neg, eye)
    assert covered.sum() > 0
    (tw, th), counts = rtm.bin_plan(scenes.Scene([neg], []), eye, W, H)
    ys, xs = np.nonzero(covered)
    assert (counts[ys // th, xs // tw] == 1).all()
    assert counts.sum() <= (ys.max() // th - ys.min() // th + 1) * (xs.max() // tw - xs.min() // tw + 1)


def test_validation_needs_no_device(rtm, scenes):
    abi = rtm.abi
    assert abi.RTM_MAX_SCENE_SPHERES == 65536 and abi.RTM_MAX_SPHERES == 16
    lib = rtm.load_library()
    cam = scenes.eye_camera().to_c()
    tw, th, nt = C.c_int32(), C.c_int32(), C.c_int64()

    def call(sc, counts=None, capacity=0):
        return lib.rtm_bin_plan(C.byref(sc), C.byref(cam), W, H, C.byref(tw), C.byref(th), counts, capacity,
                                C.byref(nt))

    # capacity 0: the tile count and shape only
    sc, keep = scenes.sphere_field(17).to_c()
    assert call(sc) == abi.RTM_OK
    assert (tw.value, th.value) == (64, 8) and nt.value == 4 * 17
    # one sphere past the limit
    sc.n_spheres = abi.RTM_MAX_SCENE_SPHERES + 1
    assert call(sc) == abi.RTM_ERR_INVALID
    assert b"65536" in lib.rtm_last_error()
    # an id equal to n
    bad = scenes.sphere_field(17)
    bad.spherePrimitives[5].id = 17
    sc, keep = bad.to_c()
    assert call(sc) == abi.RTM_ERR_INVALID
    # what the binned path does not take is refused before any device work
    with_plane = scenes.sphere_field(17)
    with_plane.circlePlanePrimitives = scenes.raytracing_plane0(True).circlePlanePrimitives
    sc, keep = with_plane.to_c()
    assert sc.n_circle_planes > 0
    assert call(sc) == abi.RTM_ERR_UNSUPPORTED
    assert b"RTM_MAX_SPHERES" in lib.rtm_last_error()
    sc, keep = scenes.sphere_field(17).to_c()
    cam = scenes.perspective_eye_camera().to_c()
    assert call(sc) == abi.RTM_ERR_UNSUPPORTED
    # rtm_render_ex validates such a scene before it looks for a device
    out = (C.c_float * (4 * 4 * 4))()
    e, s = scenes.eye_camera().to_c(), scenes.shadow_camera().to_c()
    assert lib.rtm_render_ex(C.byref(sc), C.byref(cam), C.byref(s), 4, 4, 1, 0, 0, out) == abi.RTM_ERR_UNSUPPORTED
    assert b"RTM_MAX_SPHERES" in lib.rtm_last_error()
    rc = lib.rtm_render_ex(C.byref(sc), C.byref(e), C.byref(s), 4, 4, 1, 0, 0, out)
    assert rc == (abi.RTM_OK if lib.rtm_device_count() > 0 else abi.RTM_ERR_NO_DEVICE)
    # rtm_render, the ABI v1 call, keeps the answer it always gave to a 17th sphere
    assert lib.rtm_render(C.byref(sc), C.byref(e), C.byref(s), 4, 4, 1, 0, out) == abi.RTM_ERR_INVALID
    assert b"rtm_render_ex" in lib.rtm_last_error()


def test_sphere_field_and_oracle_golden_hash(scenes, oracle):
    """A tripwire for the generator and the oracle on this platform (the GPU tests compare
    with the oracle itself, not with this hash)."""
    rgba = oracle.render(scenes.sphere_field(300), scenes.eye_camera(), scenes.shadow_camera(), W, H, 32, 0)["rgba"]
    want = json.load(open(GOLDEN))["sphere_field_300_200x136_k32_rgba_sha256"]
    assert hashlib.sha256(np.ascontiguousarray(rgba).tobytes()).hexdigest() == want
