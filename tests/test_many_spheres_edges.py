"""The binned sphere path on the GPU, directed cases off the beaten track of
tests/test_many_spheres.py: tile lists whose lengths sit on the fill kernel's 64-entry
chunk seams with the LAST entry the winner (and coincident spheres whose ties the FIRST
must win), degenerate spheres (negative, zero, NaN,
infinite, denormal-small radii; NaN, infinite and 1e300 positions) and duplicate ids on
the device, a tilted sun and a translated eye, 0 and 4 patches at 1 and 250 march steps,
row parts in the byte formats with guard bytes, tile grids 65 tiles wide and 251 tile rows
high, the 65536-sphere limit, the refusal of lists past 2^31-1 entries, the upload ring
wrapping while the device is a whole ring behind the host, and two contexts at once.

Every case first asserts on the ORACLE's own output that it cannot pass vacuously (hit
pixels, finite shadow texels, the plan's list lengths -- the values observed when the case
was written, so a change to scenes.sphere_field or to the oracle fails a precondition
instead of silently weakening the case); then the GPU frame and shadow map equal the
oracle's bit for bit, and rtm_ctx_oob_reads stays 0 (the autouse fixture of
test_many_spheres)."""
import dataclasses
import math

import numpy as np
import pytest

from conftest import bits_equal, device_smap, first_mismatch
from test_bounds import oob
from test_many_spheres_host import moved_eye, refusal_scene, stack
from test_many_spheres import K, check, hit_pixels, no_out_of_range_reads, render, want  # noqa: F401 (fixture)
from test_stale_state_fuzz import _patch_sets

pytestmark = pytest.mark.gpu

W, H = 200, 136


def finite_texels(ref):
    return int(np.isfinite(ref["shadow"]).sum())


def plan_counts(rtm, scenes, scene, w, h, eye=None, sh=None):
    return tuple(rtm.bin_plan(scene, cam, w, h)[1].astype(np.int64)
                 for cam in (eye or scenes.eye_camera(), sh or scenes.shadow_camera()))


# ---- chunk seams: every tile list has exactly n entries and the last one wins ----
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_chunk_seams_last_entry_wins(rtm, gpu_ctx, oracle, scenes, n):
    scene = stack(scenes, n, 5.0)
    for counts in plan_counts(rtm, scenes, scene, W, H):
        assert counts.min() == counts.max() == n
    ref = want(oracle, scenes, f"stack{n}", scene, W, H)
    last = scene.spherePrimitives[-1]
    alone = scenes.Scene([scenes.PrimitiveSphere(0, last.shading, last.pos, last.r)], [scenes.BENCH_PATCH])
    one = want(oracle, scenes, f"stack{n}_last_alone", alone, W, H)
    assert hit_pixels(scenes, ref["rgba"]) == W * H == finite_texels(ref)
    assert bits_equal(ref["rgba"], one["rgba"]) and bits_equal(ref["shadow"], one["shadow"])
    # ... and not those of the last but one (a dropped final entry shows)
    prev = scene.spherePrimitives[-2]
    before = scenes.Scene([scenes.PrimitiveSphere(0, prev.shading, prev.pos, prev.r)], [scenes.BENCH_PATCH])
    two = want(oracle, scenes, f"stack{n}_last_but_one_alone", before, W, H)
    assert int((two["rgba"] != ref["rgba"]).any(axis=2).sum()) == W * H
    assert int((two["shadow"] != ref["shadow"]).sum()) > W * H // 4  # (the patch is nearer in the other texels)
    check(gpu_ctx, oracle, scenes, f"stack{n}", scene, W, H)
    assert gpu_ctx.last_bin_refs() == (n * 4 * 17, n * 4 * 17)


@pytest.mark.parametrize("n", [65, 129])
def test_chunk_seams_first_entry_wins_ties(rtm, gpu_ctx, oracle, scenes, n):
    """n coincident spheres in every tile list, colours cycling: every depth ties, and the
    strict '<' keeps the FIRST in scene order through every later chunk ('<=' would hand
    the pixel to the last)."""
    scene = scenes.Scene([scenes.PrimitiveSphere(i, scenes.Shading(*scenes._COLORS_B[i % 3]), (0.0, 0.0, 0.0), 5.0)
                          for i in range(n)], [scenes.BENCH_PATCH])
    assert (n - 1) % 3 != 0  # (the last sphere's colour is not the first's)
    for counts in plan_counts(rtm, scenes, scene, W, H):
        assert counts.min() == counts.max() == n
    ref = want(oracle, scenes, f"coincident{n}", scene, W, H)
    assert hit_pixels(scenes, ref["rgba"]) == W * H == finite_texels(ref)

    def alone(i):
        s = scene.spherePrimitives[i]
        return scenes.Scene([scenes.PrimitiveSphere(0, s.shading, s.pos, s.r)], [scenes.BENCH_PATCH])

    first = want(oracle, scenes, "coincident_first_alone", alone(0), W, H)
    last = want(oracle, scenes, f"coincident{n}_last_alone", alone(n - 1), W, H)
    assert bits_equal(ref["rgba"], first["rgba"]) and bits_equal(ref["shadow"], first["shadow"])
    assert int((last["rgba"] != ref["rgba"]).any(axis=2).sum()) == W * H
    check(gpu_ctx, oracle, scenes, f"coincident{n}", scene, W, H)


def test_chunk_seam_partial_cover(rtm, gpu_ctx, oracle, scenes):
    """The 65-sphere stack with r = 0.6: lists of every length up to 65, spheres ending
    inside tiles, thousands of distinct pixel values."""
    scene = stack(scenes, 65, 0.6)
    ce, cs = plan_counts(rtm, scenes, scene, W, H)
    assert ce.max() == cs.max() == 65 and ce.min() == 0
    ref = want(oracle, scenes, "stack65_r0.6", scene, W, H)
    assert hit_pixels(scenes, ref["rgba"]) == 8202
    assert finite_texels(ref) > 0
    assert len(np.unique(ref["rgba"].reshape(-1, 4), axis=0)) > 1000
    check(gpu_ctx, oracle, scenes, "stack65_r0.6", scene, W, H)


# ---- degenerate spheres on the device ----
def wide_field(scenes):
    return scenes.sphere_field(40, rmin=0.05, rmax=0.2)


def degenerate_field(scenes):
    scene = wide_field(scenes)
    s = scene.spherePrimitives
    s[3].r = -s[3].r
    s[7].pos = (s[7].pos[0], math.nan, s[7].pos[2])
    s[11].r = math.inf
    s[13].r = 0.0
    s[17].r = math.nan
    s[19].pos = (s[19].pos[0], s[19].pos[1], math.inf)
    s[23].pos = (0.2, 0.0, 1e300)
    s[29].r = 1e-300
    return scene


def test_degenerate_spheres(gpu_ctx, oracle, scenes):
    plain = want(oracle, scenes, "field40_wide", wide_field(scenes), W, H)
    scene = degenerate_field(scenes)
    ref = want(oracle, scenes, "field40_wide_degenerate", scene, W, H)
    assert hit_pixels(scenes, plain["rgba"]) == 4844
    assert hit_pixels(scenes, ref["rgba"]) == 3283
    assert int((ref["rgba"] != plain["rgba"]).any(axis=2).sum()) == 2212
    assert not np.isnan(ref["rgba"]).any() and not np.isnan(ref["shadow"]).any()
    assert finite_texels(ref) > 0
    check(gpu_ctx, oracle, scenes, "field40_wide_degenerate", scene, W, H)


def test_negative_radius_alone_in_view(rtm, gpu_ctx, oracle, scenes):
    """One r = -0.3 sphere in view and 16 small ones far above the image: the binned path
    with nothing but the negative radius to draw (its depth is pos - h * r as the reference
    writes it, sign and all)."""
    white = scenes.Shading(1.0, 1.0, 1.0)
    spheres = [scenes.PrimitiveSphere(0, scenes.Shading(0.9, 0.2, 0.2), (0.0, 0.0, 0.5), -0.3)]
    spheres += [scenes.PrimitiveSphere(1 + i, white, (0.0, 5.0, 0.1 * i), 0.05) for i in range(16)]
    scene = scenes.Scene(spheres, [scenes.BENCH_PATCH])
    ce, cs = plan_counts(rtm, scenes, scene, W, H)
    assert ce.sum() == 12 and cs.sum() > 0
    ref = want(oracle, scenes, "negative_alone", scene, W, H)
    assert hit_pixels(scenes, ref["rgba"]) == 1923
    assert finite_texels(ref) > 0
    # the sign matters: the same scene with r = +0.3 has another frame and another map
    positive = [dataclasses.replace(spheres[0], r=0.3)] + spheres[1:]
    pos = want(oracle, scenes, "positive_alone", scenes.Scene(positive, [scenes.BENCH_PATCH]), W, H)
    assert not bits_equal(pos["rgba"], ref["rgba"]) and not bits_equal(pos["shadow"], ref["shadow"])
    check(gpu_ctx, oracle, scenes, "negative_alone", scene, W, H)


def test_duplicate_ids(gpu_ctx, oracle, scenes):
    """Every sphere carries id 5: every hit is shaded as spherePrimitives[5]."""
    ident = want(oracle, scenes, "field40_wide", wide_field(scenes), W, H)["rgba"]
    scene = wide_field(scenes)
    for s in scene.spherePrimitives:
        s.id = 5
    ref = want(oracle, scenes, "field40_wide_ids5", scene, W, H)
    assert int((ref["rgba"] != ident).any(axis=2).sum()) == hit_pixels(scenes, ident) == 4844
    check(gpu_ctx, oracle, scenes, "field40_wide_ids5", scene, W, H)


# ---- cameras ----
@pytest.mark.parametrize("w,h", [(200, 136), (65, 9)])
@pytest.mark.parametrize("cams", ["tilted_sun", "moved_eye", "both"])
def test_cameras(rtm, gpu_ctx, oracle, scenes, cams, w, h):
    """A sun that shines along no axis (shadow_texel's general per-step march, shadow pixel
    ranges elsewhere) and an eye translated off the axes."""
    eye = moved_eye(scenes) if cams != "tilted_sun" else None
    sh = scenes.tilted_shadow_camera() if cams != "moved_eye" else None
    scene = scenes.sphere_field(300)
    ref = want(oracle, scenes, "field300", scene, w, h, eye=eye, sh=sh)
    base = want(oracle, scenes, "field300", scene, w, h)
    assert hit_pixels(scenes, ref["rgba"]) > 0 and finite_texels(ref) > 0
    assert not bits_equal(ref["rgba"], base["rgba"])
    if sh is not None:
        assert not bits_equal(ref["shadow"], base["shadow"])
    check(gpu_ctx, oracle, scenes, "field300", scene, w, h, eye=eye, sh=sh)
    plan = tuple(int(c.sum()) for c in plan_counts(rtm, scenes, scene, w, h, eye, sh))
    assert gpu_ctx.last_bin_refs() == plan and min(plan) > 0


# ---- patches and march steps ----
@pytest.mark.parametrize("k", [1, 250])
@pytest.mark.parametrize("npatch", [0, 4])
def test_patches_and_steps(gpu_ctx, oracle, scenes, npatch, k):
    patches = [] if npatch == 0 else [scenes.BENCH_PATCH, scenes.SCENE_B_PATCH2, scenes.REFERENCE_PATCH,
                                      _patch_sets(scenes)[4][0]]
    assert len(patches) == npatch
    scene = scenes.sphere_field(60, patches=patches)
    ref = want(oracle, scenes, f"field60_patches{npatch}", scene, W, H, k)
    one = want(oracle, scenes, "field60", scenes.sphere_field(60), W, H, k)
    assert hit_pixels(scenes, ref["rgba"]) > 0 and finite_texels(ref) > 0
    if k > 1:  # (one march step of these patches crosses nothing)
        assert not bits_equal(ref["shadow"], one["shadow"])
    check(gpu_ctx, oracle, scenes, f"field60_patches{npatch}", scene, W, H, k)


# ---- row parts in the byte formats ----
@pytest.mark.parametrize("pad", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("w", [200, 65], ids=["w200", "w65"])
@pytest.mark.parametrize("fmt", [1, 2], ids=["rgba8", "rgb8"])
def test_rows_in_byte_formats(rtm, gpu_ctx, oracle, scenes, fmt, w, pad):
    """row_begin > 0 with RGBA8 / RGB8 (W = 200: dword stores when the base is aligned;
    W = 65: bytes), each part between guard bytes that must stay as they were."""
    import torch
    h = H
    scene = scenes.sphere_field(300)
    ref32 = want(oracle, scenes, "field300", scene, w, h)["rgba"]
    assert hit_pixels(scenes, ref32) > 0
    rgb = oracle.encode_rgb8(ref32).astype(np.uint8)
    ref = rgb if fmt == 2 else np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], -1)
    nb = rtm.abi.FORMAT_BYTES[fmt]
    lead = 16 + (4 * pad if fmt == 1 else pad)  # (as test_formats offsets its bases)
    parts = []
    for b0, b1 in ((0, 1), (1, 50), (50, h), (h - 1, h)):
        n = (b1 - b0) * w * nb
        raw = torch.full((lead + n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        out = raw[lead:lead + n]
        assert out.data_ptr() % 4 == (0 if fmt == 1 else pad)
        torch.cuda.synchronize()
        gpu_ctx.render_rows_async(scene, scenes.eye_camera(), scenes.shadow_camera(), w, h, K, 0, fmt,
                                  out.data_ptr(), b0, b1)
        gpu_ctx.synchronize()
        assert gpu_ctx.last_sphere_path() == 1
        got = raw.cpu().numpy()
        assert (got[:lead] == 0xA5).all() and (got[lead + n:] == 0xA5).all(), f"rows [{b0},{b1}): guard bytes written"
        parts.append(got[lead:lead + n].reshape(b1 - b0, w, nb))
    assert np.array_equal(parts[3], ref[h - 1:h])
    got = np.concatenate(parts[:3], 0)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"


# ---- tile-grid shapes ----
@pytest.mark.parametrize("w,h", [(4097, 3), (3, 2001)])
def test_tile_grid_shapes(rtm, gpu_ctx, oracle, scenes, w, h):
    """65 tiles across (one past a wave of tiles) and 251 tile rows."""
    scene = scenes.sphere_field(300)
    ce, cs = plan_counts(rtm, scenes, scene, w, h)
    assert ce.shape == cs.shape == ((1, 65) if w == 4097 else (251, 1))
    ref = want(oracle, scenes, "field300", scene, w, h)
    assert hit_pixels(scenes, ref["rgba"]) > 0 and finite_texels(ref) > 0
    check(gpu_ctx, oracle, scenes, "field300", scene, w, h)
    assert gpu_ctx.last_bin_refs() == (int(ce.sum()), int(cs.sum()))


# ---- the limits ----
def test_the_limit(rtm, gpu_ctx, oracle, scenes):
    """RTM_MAX_SCENE_SPHERES spheres render; one more is RTM_ERR_INVALID."""
    import torch
    w, h = 128, 72
    n = rtm.abi.RTM_MAX_SCENE_SPHERES
    assert n == 65536
    scene = scenes.sphere_field(n, rmax=0.03)
    ce, cs = plan_counts(rtm, scenes, scene, w, h)
    assert ce.max() == 4726
    ref = want(oracle, scenes, "field65536", scene, w, h)
    assert hit_pixels(scenes, ref["rgba"]) > 0 and finite_texels(ref) > 0
    check(gpu_ctx, oracle, scenes, "field65536", scene, w, h)
    assert gpu_ctx.last_bin_refs() == (int(ce.sum()), int(cs.sum()))
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(rtm.RtmError) as e:
        gpu_ctx.render_async(scenes.sphere_field(n + 1, rmax=0.03), scenes.eye_camera(), scenes.shadow_camera(), w, h,
                             K, 0, out.data_ptr())
    assert e.value.code == rtm.abi.RTM_ERR_INVALID and "65536" in str(e.value)


def test_list_size_refusal(rtm, gpu_ctx, oracle, scenes):
    """64800 tiles x 65536 spheres > 2^31-1 list entries: RTM_ERR_OOM before any device
    work, and the context renders the next frame as if nothing had happened."""
    import torch
    w, h = 7680, 4320
    assert (-(-w // 64)) * (-(-h // 8)) * 65536 > 2 ** 31 - 1
    out = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")  # (full size: a frame that did run stays in it)
    with pytest.raises(rtm.RtmError) as e:
        gpu_ctx.render_async(refusal_scene(scenes), scenes.eye_camera(), scenes.shadow_camera(), w, h, K, 0,
                             out.data_ptr())
    assert e.value.code == rtm.abi.RTM_ERR_OOM and "2^31-1" in str(e.value), str(e.value)
    assert gpu_ctx.last_bin_refs() == (0, 0)
    del out
    got = check(gpu_ctx, oracle, scenes, "field17", scenes.sphere_field(17), W, H)
    assert hit_pixels(scenes, got) == 322


# ---- the upload ring with the device a whole ring behind the host ----
def test_ring_wraps_while_the_device_is_behind(rtm, gpu_ctx, oracle, scenes):
    """Nine binned frames enqueued while the context's stream is still busy with earlier
    work (a few milliseconds of a spinning kernel): the host runs a whole ring ahead of
    the device, so a slot's pinned staging may be refilled only once the upload that read
    it has run (ring_slot's wait on copied[j]).  Without that wait the first frames are
    rendered from a later frame's tables.  The slots are sized by four frames of the
    largest scene first, so nothing in the timed call regrows a slot (which would wait
    for the device)."""
    import torch
    eye, sh = scenes.eye_camera(), scenes.shadow_camera()
    ns = [17, 33, 64, 65, 129, 18, 40, 300, 20]
    frames = [scenes.sphere_field(n) for n in ns]
    refs = [want(oracle, scenes, f"field{n}", frames[i], W, H)["rgba"] for i, n in enumerate(ns)]
    assert all(hit_pixels(scenes, r) > 0 for r in refs)
    assert all(not bits_equal(refs[i], refs[j]) for i in range(9) for j in range(i))
    outs = [torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in ns]
    torch.cuda.synchronize()
    gpu_ctx.render_frames_async([frames[7]] * 4, eye, sh, W, H, K, 0, [o.data_ptr() for o in outs[:4]])
    gpu_ctx.synchronize()
    prepared = gpu_ctx.prepare_frames(frames)
    with torch.cuda.stream(torch.cuda.ExternalStream(gpu_ctx.stream)):
        torch.cuda._sleep(20_000_000)
    gpu_ctx.render_frames_async(frames, eye, sh, W, H, K, 0, [o.data_ptr() for o in outs], prepared=prepared)
    gpu_ctx.synchronize()
    assert gpu_ctx.last_sphere_path() == 1
    for i, r in enumerate(refs):
        got = outs[i].cpu().numpy()
        assert bits_equal(got, r), (i, ns[i], first_mismatch(got, r))
    m = device_smap(gpu_ctx, W, H)
    last = want(oracle, scenes, "field20", frames[8], W, H)["shadow"]
    assert bits_equal(m, last), first_mismatch(m, last)


# ---- two contexts ----
def test_two_contexts(rtm, gpu_ctx, oracle, scenes):
    """Binned frames of different sizes and sphere counts alternating on two contexts of
    one device, nothing waited for in between: each context's ring is its own."""
    import torch
    other = rtm.Context(0)
    try:
        jobs = [("field300", 300, 200, 136), ("field60", 60, 200, 136), ("field300", 300, 65, 9),
                ("field17", 17, 200, 136), ("field300", 300, 200, 136), ("field60", 60, 200, 136),
                ("field17", 17, 200, 136), ("field300", 300, 65, 9), ("field60", 60, 200, 136),
                ("field300", 300, 200, 136)]
        eye, sh = scenes.eye_camera(), scenes.shadow_camera()
        refs = [want(oracle, scenes, key, scenes.sphere_field(n), w, h) for key, n, w, h in jobs]
        assert all(hit_pixels(scenes, r["rgba"]) > 0 for r in refs)
        outs = [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _, _, w, h in jobs]
        torch.cuda.synchronize()
        assert oob(rtm, other) >= 0
        for i, (key, n, w, h) in enumerate(jobs):
            ctx = (gpu_ctx, other)[i % 2]
            ctx.render_async(scenes.sphere_field(n), eye, sh, w, h, K, 0, outs[i].data_ptr())
        gpu_ctx.synchronize()
        other.synchronize()
        assert gpu_ctx.last_sphere_path() == other.last_sphere_path() == 1
        for i, r in enumerate(refs):
            got = outs[i].cpu().numpy()
            assert bits_equal(got, r["rgba"]), (i, jobs[i], first_mismatch(got, r["rgba"]))
        for ctx, i in ((gpu_ctx, len(jobs) - 2), (other, len(jobs) - 1)):
            m = device_smap(ctx, jobs[i][2], jobs[i][3])
            assert bits_equal(m, refs[i]["shadow"]), (i, first_mismatch(m, refs[i]["shadow"]))
        assert oob(rtm, other) == 0
    finally:
        other.close()
