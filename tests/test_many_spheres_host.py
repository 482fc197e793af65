"""The binned sphere path's host side (CPU): rtm_bin_plan -- the code the render path
sizes and fills its per-tile sphere lists from -- checked against the oracle's own
rasterizer, its treatment of spheres that cover nothing, validation without a device,
and one golden hash that pins scenes.sphere_field and the oracle on this platform."""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

W, H = 200, 136
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_spheres.json")


def _covered(oracle, scenes, sphere, cam):
    """Pixels the oracle's rasterizer covers with `sphere` alone (either face)."""
    one = scenes.Scene([scenes.PrimitiveSphere(0, sphere.shading, sphere.pos, sphere.r)], [])
    m = np.zeros((H, W), bool)
    for face in (scenes.EnumFace.FRONT, scenes.EnumFace.BACK):
        vp = oracle.Viewport(W, H, face, cam)
        vp.rasterize(one)
        m |= np.isfinite(vp.zbuffer())
    return m


def _cover_counts(oracle, scenes, scene, cam, tw, th, shape):
    """Per tile: the spheres covering a pixel of it, and the spheres whose covered
    bounding box, grown by one tile on every side, reaches it."""
    cover = np.zeros(shape, np.int64)
    box = np.zeros(shape, np.int64)
    for s in scene.spherePrimitives:
        ys, xs = np.nonzero(_covered(oracle, scenes, s, cam))
        if len(ys) == 0:
            continue
        for ty, tx in set(zip((ys // th).tolist(), (xs // tw).tolist())):
            cover[ty, tx] += 1
        box[max(ys.min() // th - 1, 0):ys.max() // th + 2, max(xs.min() // tw - 1, 0):xs.max() // tw + 2] += 1
    return cover, box


@pytest.mark.parametrize("cam", ["eye", "shadow"])
def test_bin_plan_is_conservative_and_culls(rtm, scenes, oracle, cam):
    camera = scenes.eye_camera() if cam == "eye" else scenes.shadow_camera()
    scene = scenes.sphere_field(300)
    (tw, th), counts = rtm.bin_plan(scene, camera, W, H)
    assert counts.shape == (-(-H // th), -(-W // tw))
    cover, box = _cover_counts(oracle, scenes, scene, camera, tw, th, counts.shape)
    assert cover.sum() > 0
    assert (counts >= cover).all(), "a tile's list misses a sphere that covers a pixel of it"
    # the cull must bite: the bound holds for the reference's own bounding boxes plus a
    # tile of margin (checked here, so the bound is not one only the plan could meet)
    bound = len(scene.spherePrimitives) * counts.size / 4
    assert box.sum() < bound
    assert counts.sum() < bound
    assert counts.sum() <= box.sum()


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
