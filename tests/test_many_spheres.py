"""The binned sphere path on the GPU: scenes of more than RTM_MAX_SPHERES spheres (device
sphere tables + per-tile lists in scene order) against the CPU oracle, bit for bit: the
RGBA32F frame and the shadow viewport's zBuffer (rtm_ctx_shadow_map).  After every test
the device's count of out-of-range table reads must be 0."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import bits_equal, device_smap, first_mismatch

pytestmark = pytest.mark.gpu

NT = min(8, os.cpu_count() or 1)
W, H, K = 200, 136, 32


@pytest.fixture(autouse=True)
def no_out_of_range_reads(rtm, gpu_ctx):
    yield
    n = C.c_int64(-1)
    lib = rtm.load_library()
    assert lib.rtm_ctx_oob_reads(gpu_ctx.handle, C.byref(n)) == 0
    assert n.value == 0, f"{n.value} out-of-range table reads"


_oracle_cache = {}


def _cam_key(cam):
    return None if cam is None else (tuple(cam.position), tuple(cam.dirNormalized), tuple(cam.upNormalized),
                                     tuple(cam.sideNormalized))


def want(oracle, scenes, key, scene, w, h, k=K, flags=0, eye=None, sh=None):
    """The oracle frame + shadow map of a named case, computed once per session (eye, sh:
    other cameras than eye_camera() and shadow_camera())."""
    key = (key, w, h, k, flags, _cam_key(eye), _cam_key(sh))
    if key not in _oracle_cache:
        r = oracle.render(scene, eye or scenes.eye_camera(), sh or scenes.shadow_camera(), w, h, k, flags, nthreads=NT,
                          want_shadow=True)
        r["rgba"].setflags(write=False)
        r["shadow"].setflags(write=False)
        _oracle_cache[key] = r
    return _oracle_cache[key]


def render(gpu_ctx, scenes, scene, w, h, k=K, flags=0, eye=None, sh=None):
    import torch
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.render_async(scene, eye or scenes.eye_camera(), sh or scenes.shadow_camera(), w, h, k, flags,
                         out.data_ptr())
    gpu_ctx.synchronize()
    return out.cpu().numpy()


def check(gpu_ctx, oracle, scenes, key, scene, w, h, k=K, flags=0, path=1, eye=None, sh=None):
    ref = want(oracle, scenes, key, scene, w, h, k, flags, eye, sh)
    got = render(gpu_ctx, scenes, scene, w, h, k, flags, eye, sh)
    assert gpu_ctx.last_sphere_path() == path
    assert bits_equal(got, ref["rgba"]), first_mismatch(got, ref["rgba"])
    smap = device_smap(gpu_ctx, w, h)
    assert bits_equal(smap, ref["shadow"]), first_mismatch(smap, ref["shadow"])
    return got


def hit_pixels(scenes, rgba):
    return int((rgba != np.array([0.0, 0.2, 0.2, 1.0], np.float32)).any(axis=2).sum())


def test_the_boundary(rtm, gpu_ctx, oracle, scenes):
    """16 spheres take the kernel-argument path, 17 the binned one; both exact."""
    check(gpu_ctx, oracle, scenes, "scene_b", scenes.scene_b(), W, H, path=0)
    got = check(gpu_ctx, oracle, scenes, "field17", scenes.sphere_field(17), W, H, path=1)
    assert hit_pixels(scenes, got) == 322
    assert gpu_ctx.shadow_map_texel_bytes() == 8


@pytest.mark.parametrize("w,h", [(200, 136), (1, 1), (65, 9), (64, 8), (1000, 7)])
def test_ragged_sizes(gpu_ctx, oracle, scenes, w, h):
    """Widths and heights that are no tile multiples, one partial tile, one tile exactly."""
    check(gpu_ctx, oracle, scenes, "field300", scenes.sphere_field(300), w, h)


def _pairs(scenes, swapped):
    red, green = scenes.Shading(0.9, 0.2, 0.2), scenes.Shading(0.2, 0.9, 0.2)
    spheres = []
    for p in scenes.sphere_field(20, rmin=0.05, rmax=0.2).spherePrimitives:
        for sh in ((green, red) if swapped else (red, green)):
            spheres.append(scenes.PrimitiveSphere(len(spheres), sh, p.pos, p.r))
    return scenes.Scene(spheres, [scenes.BENCH_PATCH])


def test_scene_order_on_ties(gpu_ctx, oracle, scenes):
    """Coincident spheres tie on depth at every pixel: the first in scene order wins."""
    a = check(gpu_ctx, oracle, scenes, "pairs", _pairs(scenes, False), W, H)
    b = check(gpu_ctx, oracle, scenes, "pairs_swapped", _pairs(scenes, True), W, H)
    differ = int((a != b).any(axis=2).sum())
    assert differ == hit_pixels(scenes, a) == 3014  # an order bug cannot hide


def test_id_is_not_the_index(gpu_ctx, oracle, scenes):
    """The reference shades spherePrimitives[id]: with id = n-1-i a hit takes another
    sphere's position, radius and colour."""
    scene = scenes.sphere_field(40, rmin=0.05, rmax=0.2)
    ident = want(oracle, scenes, "field40_wide", scene, W, H)["rgba"]
    rev = scenes.sphere_field(40, rmin=0.05, rmax=0.2)
    for i, s in enumerate(rev.spherePrimitives):
        s.id = 39 - i
    got = check(gpu_ctx, oracle, scenes, "field40_wide_reversed_ids", rev, W, H)
    assert int((got != ident).any(axis=2).sum()) == hit_pixels(scenes, ident) == 4844


def _pile(scenes):
    u = scenes.splitmix64(7)
    spheres = []
    for i in range(200):
        x = -0.3 + 0.6 * next(u)
        y = -0.2 + 0.4 * next(u)
        z = 0.3 + 0.4 * next(u)
        r = 0.5 + 0.3 * next(u)
        spheres.append(scenes.PrimitiveSphere(i, scenes.Shading(*scenes._COLORS_B[i % 4]), (x, y, z), r))
    return scenes.Scene(spheres, [scenes.BENCH_PATCH])


@pytest.mark.parametrize("w,h", [(64, 8), (200, 136)])
def test_lists_longer_than_one_chunk(rtm, gpu_ctx, oracle, scenes, w, h):
    """200 large spheres piled over the image centre: a tile's list passes 64 entries, the
    fill kernel's chunk."""
    scene = _pile(scenes)
    for cam in (scenes.eye_camera(), scenes.shadow_camera()):
        assert rtm.bin_plan(scene, cam, w, h)[1].max() > 64
    check(gpu_ctx, oracle, scenes, "pile", scene, w, h)


def test_many(rtm, gpu_ctx, oracle, scenes):
    scene = scenes.sphere_field(1024)
    w, h = 256, 192
    check(gpu_ctx, oracle, scenes, "field1024", scene, w, h)
    plan = tuple(int(rtm.bin_plan(scene, cam, w, h)[1].sum()) for cam in (scenes.eye_camera(), scenes.shadow_camera()))
    assert gpu_ctx.last_bin_refs() == plan and min(plan) > 0


def test_host_output(rtm, oracle, scenes):
    """rtm_render_ex: the blocking host-output form, on the default context."""
    ref = want(oracle, scenes, "field17", scenes.sphere_field(17), W, H)["rgba"]
    got = rtm.render_frame_ex(scenes.sphere_field(17), scenes.eye_camera(), scenes.shadow_camera(), W, H, K, 0)
    assert bits_equal(got, ref), first_mismatch(got, ref)


def test_threaded_table_build(gpu_ctx, oracle, scenes):
    """From 2048 spheres the host projects the spheres on several threads: the same tables."""
    check(gpu_ctx, oracle, scenes, "field2048", scenes.sphere_field(2048, rmax=0.03), 128, 72)


@pytest.mark.parametrize("flags", [1, 2, 3, 4], ids=["no_march", "no_shadow_raster", "neither", "fused_shadow"])
def test_flags(gpu_ctx, oracle, scenes, flags):
    ref = want(oracle, scenes, "field60", scenes.sphere_field(60), W, H, K, flags)
    got = render(gpu_ctx, scenes, scenes.sphere_field(60), W, H, K, flags)
    assert gpu_ctx.last_sphere_path() == 1
    assert bits_equal(got, ref["rgba"]), first_mismatch(got, ref["rgba"])
    # (a fused frame's map is materialised all the same; the oracle's shadow viewport is
    # the same with or without the flag)
    smap = device_smap(gpu_ctx, W, H)
    assert bits_equal(smap, ref["shadow"]), first_mismatch(smap, ref["shadow"])


def test_rows(rtm, gpu_ctx, oracle, scenes):
    import torch
    scene = scenes.sphere_field(300)
    ref = want(oracle, scenes, "field300", scene, W, H)["rgba"]
    parts = []
    for b0, b1 in ((0, 1), (1, 50), (50, H)):
        out = torch.empty((b1 - b0, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu_ctx.render_rows_async(scene, scenes.eye_camera(), scenes.shadow_camera(), W, H, K, 0,
                                  rtm.abi.RTM_FORMAT_RGBA32F, out.data_ptr(), b0, b1)
        gpu_ctx.synchronize()
        parts.append(out.cpu().numpy())
    got = np.concatenate(parts, 0)
    assert bits_equal(got, ref), first_mismatch(got, ref)


@pytest.mark.parametrize("w,h", [(200, 136), (65, 9)])
@pytest.mark.parametrize("fmt", [1, 2], ids=["rgba8", "rgb8"])
def test_formats(rtm, gpu_ctx, oracle, scenes, fmt, w, h):
    import torch
    scene = scenes.sphere_field(300)
    rgb = oracle.encode_rgb8(want(oracle, scenes, "field300", scene, w, h)["rgba"]).astype(np.uint8)
    ref = rgb if fmt == 2 else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], -1)
    nb = rtm.abi.FORMAT_BYTES[fmt]
    for pad in (0, 1):  # (RGB8: dword stores where W % 4 == 0 and the base is aligned, else bytes)
        raw = torch.zeros(h * w * nb + 4, dtype=torch.uint8, device="cuda")
        out = raw[4 * pad if fmt == 1 else pad:][:h * w * nb]
        torch.cuda.synchronize()
        gpu_ctx.render_rows_async(scene, scenes.eye_camera(), scenes.shadow_camera(), w, h, K, 0, fmt, out.data_ptr())
        gpu_ctx.synchronize()
        got = out.cpu().numpy().reshape(h, w, nb)
        assert np.array_equal(got, ref), f"pad {pad}: {int((got != ref).sum())} bytes differ"
    host = rtm.render_frame_ex(scene, scenes.eye_camera(), scenes.shadow_camera(), w, h, K, 0, fmt)
    assert np.array_equal(host, ref)


def _moving(scenes, frame):
    """sphere_field(40) whose sphere 0 moves as closely_orbiting_sphere moves its third."""
    scene = scenes.sphere_field(40)
    orbit = scenes.closely_orbiting_sphere(frame).spherePrimitives[2]
    scene.spherePrimitives[0].pos = orbit.pos
    scene.spherePrimitives[0].r = orbit.r
    return scene


def test_frame_sequence(gpu_ctx, oracle, scenes):
    import torch
    eye, sh = scenes.eye_camera(), scenes.shadow_camera()
    frames = [_moving(scenes, 40 * f) for f in range(4)]
    refs = [want(oracle, scenes, f"moving{f}", frames[f], W, H)["rgba"] for f in range(4)]
    assert all(not bits_equal(refs[0], r) for r in refs[1:])
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    gpu_ctx.render_frames_async(frames, eye, sh, W, H, K, 0, [o.data_ptr() for o in outs])
    gpu_ctx.synchronize()
    assert gpu_ctx.last_sphere_path() == 1 and gpu_ctx.last_batch() == 1 and gpu_ctx.last_lanes() == 1
    for f in range(4):
        got = outs[f].cpu().numpy()
        assert bits_equal(got, refs[f]), (f, first_mismatch(got, refs[f]))
    # one repeated output pointer: the last frame wins
    gpu_ctx.render_frames_async(frames, eye, sh, W, H, K, 0, [outs[0].data_ptr()] * 4)
    gpu_ctx.synchronize()
    got = outs[0].cpu().numpy()
    assert bits_equal(got, refs[3]), first_mismatch(got, refs[3])
    # a 3-sphere and a 40-sphere scene alternating: each frame on its own path, each exact
    small = scenes.scene_a_bench(100)
    mixed = [small, frames[1], small, frames[2]]
    mrefs = [want(oracle, scenes, "a_bench100", small, W, H)["rgba"], refs[1]]
    mrefs += [mrefs[0], refs[2]]
    gpu_ctx.render_frames_async(mixed, eye, sh, W, H, K, 0, [o.data_ptr() for o in outs])
    gpu_ctx.synchronize()
    assert gpu_ctx.last_sphere_path() == 1
    for f in range(4):
        got = outs[f].cpu().numpy()
        assert bits_equal(got, mrefs[f]), (f, first_mismatch(got, mrefs[f]))
    gpu_ctx.render_frames_async([frames[0], small], eye, sh, W, H, K, 0, [outs[0].data_ptr(), outs[1].data_ptr()])
    gpu_ctx.synchronize()
    assert gpu_ctx.last_sphere_path() == 0
    assert bits_equal(outs[1].cpu().numpy(), mrefs[0])


def test_refusals(rtm, gpu_ctx, scenes):
    """More than RTM_MAX_SPHERES spheres off the binned path: RTM_ERR_UNSUPPORTED with a
    message that names the limit -- not a crash, not RTM_ERR_INVALID."""
    import torch
    abi = rtm.abi
    scene, eye, sh = scenes.sphere_field(17), scenes.eye_camera(), scenes.shadow_camera()
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    with_plane = scenes.sphere_field(17)
    with_plane.circlePlanePrimitives = scenes.raytracing_plane0(True).circlePlanePrimitives[:1]
    vp = rtm.Viewport(gpu_ctx, W, H, scenes.EnumFace.FRONT, eye)
    calls = {
        "perspective eye": lambda: gpu_ctx.render_async(scene, scenes.perspective_eye_camera(), sh, W, H, K, 0,
                                                        out.data_ptr()),
        "circle plane": lambda: gpu_ctx.render_async(with_plane, eye, sh, W, H, K, 0, out.data_ptr()),
        "stripes": lambda: gpu_ctx.render_stripes_async(scene, eye, sh, W, H, K, 0, abi.RTM_FORMAT_RGBA32F, 8, 2, 0,
                                                        out.data_ptr()),
        "stats": lambda: gpu_ctx.stats(scene, eye, sh, W, H, K),
        "Viewport.rasterize": lambda: vp.rasterize(scene),
        "render_frame_multi": lambda: rtm.render_frame_multi(scene, eye, sh, W, H, K, 0, n_gpus=1),
    }
    try:
        for name, call in calls.items():
            with pytest.raises(rtm.RtmError) as e:
                call()
            assert e.value.code == abi.RTM_ERR_UNSUPPORTED, name
            assert "RTM_MAX_SPHERES (16)" in str(e.value), (name, str(e.value))
    finally:
        vp.close()
    # the limits that stay RTM_ERR_INVALID
    bad = scenes.sphere_field(17)
    bad.spherePrimitives[3].id = 17
    with pytest.raises(rtm.RtmError) as e:
        gpu_ctx.render_async(bad, eye, sh, W, H, K, 0, out.data_ptr())
    assert e.value.code == abi.RTM_ERR_INVALID
