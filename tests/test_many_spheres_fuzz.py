"""State carried across frames of the binned sphere path: seeded random sequences of
render calls on ONE reused context, frame by frame against the oracle -- the scheme of
tests/test_stale_state_fuzz.py (which draws 0-16 spheres and never reaches this path),
over everything a context keeps between binned frames:

  * the 4-slot upload ring (enqueue_binned_frame / ring_slot): calls of up to 9 frames,
    one call of 9 binned frames per chunk (every slot reused at least twice), sphere
    counts from {0, 3, 16, 17, 18, 33, 64, 65, 300, 600, 1100, 2048} per frame, so slots
    grow, a regrown slot is reused by a smaller frame, frames move between the
    kernel-argument path and the binned path in both directions, and 2048 spheres take
    the threaded table build;
  * spheres off both viewports, covering the whole map, ordinary, and with r < 0; ids
    permuted;
  * patch sets (0 to 2 patches) changing between calls and mid-call: the march tables are
    rebuilt on a context that holds ring slots;
  * shadow_camera() or tilted_shadow_camera() (the general per-step march), eye_camera()
    or the same eye translated;
  * image sizes (the shadow map and the tables are re-sized between binned frames), 1 to
    250 march steps, every flag combination;
  * rtm_render_frames_async, rtm_render_async and rtm_render_rows_async (a row part);
  * every frame of a call into one output (the last frame must land last);
  * forced lanes and frames per launch: a call with any scene of more than 16 spheres
    still runs one lane, one frame per launch.

After every call: every frame's RGBA f32 image and the last frame's shadow map equal the
oracle's bit for bit, rtm_ctx_oob_reads == 0, rtm_ctx_last_sphere_path says which path the
last frame took, and after a binned last frame rtm_ctx_last_bin_refs equals the sums of
rtm_bin_plan for both cameras.  Seeded splitmix64: the same sequence on every run; chunk c
replays the draws of chunks 0 .. c-1, so a chunk is reproducible alone."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import bits_equal, first_mismatch
from test_bounds import oob
from test_stale_state_fuzz import SplitMix64, _patch_sets, _smap

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)
SEED = 0x2018_B1
N_CALLS = 10  # per chunk
NS = [0, 3, 16, 17, 18, 33, 64, 65, 300, 600, 1100, 2048]
BINNED = [n for n in NS if n > 16]
SIZES = [(256, 192), (200, 136), (384, 100), (130, 70), (65, 9)]
STEPS = [1, 8, 64, 250]
FLAGS = [0, 0, 0, 1, 2, 3, 4]
FUSED = 4


def _sphere(scenes, rng, n: int, sid: int):
    col = scenes.Shading(rng.uniform(0.02, 1.0), rng.uniform(0.02, 1.0), rng.uniform(0.02, 1.0))
    kind = rng.below(100)
    if kind < 25:  # off the shadow map and off the eye's view (the existing fuzz's "off")
        y = rng.pick([-1.0, 1.0]) * rng.uniform(1.6, 3.0)
        return scenes.PrimitiveSphere(sid, col, (rng.uniform(-3.0, 3.0), y, rng.uniform(-0.8, 0.8)), 0.2)
    if kind < (28 if n <= 64 else 26):  # covers every texel of the map: in every tile's list
        return scenes.PrimitiveSphere(sid, col, (0.0, 0.0, rng.uniform(1.5, 2.5)), rng.uniform(2.0, 3.0))
    pos = (rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9))
    r = rng.uniform(0.02, 0.35 if n <= 64 else 0.12)
    return scenes.PrimitiveSphere(sid, col, pos, -r if kind < 33 else r)  # a few percent with r < 0


def _scene(scenes, rng, n: int, patches):
    ids = list(range(n))
    for i in range(n - 1, 0, -1):  # Fisher-Yates with the seeded stream
        j = rng.below(i + 1)
        ids[i], ids[j] = ids[j], ids[i]
    return scenes.Scene([_sphere(scenes, rng, n, ids[i]) for i in range(n)], list(patches))


def _draw_call(scenes, rng, call: int, patch_sets):
    """One call of the sequence: every draw, in a fixed order."""
    c = {"call": call}
    c["w"], c["h"] = rng.pick(SIZES)
    c["k"] = rng.pick(STEPS)
    c["flags"] = rng.pick(FLAGS)
    c["tilted"] = rng.below(3) == 0
    c["moved"] = rng.below(3) == 0
    api = rng.below(7)
    c["api"] = "async" if api == 0 else "rows" if api == 1 else "frames"
    nframes = 1 + rng.below(9)
    all_binned = call % N_CALLS == 3  # the chunk's call of 9 binned frames
    if all_binned:
        c["api"], nframes = "frames", 9
    elif c["api"] != "frames":
        nframes = 1
    b0 = rng.below(c["h"])
    c["rows"] = (b0, b0 + 1 + rng.below(c["h"] - b0)) if c["api"] == "rows" else (0, c["h"])
    c["lanes"], c["batch"] = (0, 0) if rng.below(3) == 0 else (1 + rng.below(4), 1 + rng.below(8))
    c["same_out"] = rng.below(6) == 0
    ps = rng.pick(patch_sets)
    c["ns"], c["frames"] = [], []
    for _ in range(nframes):
        if rng.below(4) == 0:
            ps = rng.pick(patch_sets)  # the patch set changes mid-call
        n = rng.pick(BINNED if all_binned else NS)
        c["ns"].append(n)
        c["frames"].append(_scene(scenes, rng, n, ps))
    return c


def _describe(c):
    return (f"call {c['call']} ({c['api']}): {c['w']}x{c['h']} rows={c['rows']} K={c['k']} flags={c['flags']} "
            f"tilted_sun={c['tilted']} moved_eye={c['moved']} n={c['ns']} "
            f"patches={[len(f.patches) for f in c['frames']]} lanes={c['lanes']} batch={c['batch']} "
            f"same_out={c['same_out']}")


@pytest.mark.parametrize("chunk", range(4))
def test_random_binned_sequences_on_one_context(rtm, oracle, scenes, chunk):
    """chunk c: calls 10c .. 10c+9 of the seeded sequence, the four chunks on one context
    in order."""
    import torch
    rng = SplitMix64(SEED)
    patch_sets = _patch_sets(scenes)
    ctx = _ctx(rtm)
    binned_frames = 0
    for call in range(N_CALLS * (chunk + 1)):
        c = _draw_call(scenes, rng, call, patch_sets)
        if call < N_CALLS * chunk:
            continue  # (an earlier chunk's call: its draws keep the stream in step)
        w, h, k, flags, frames, ns = c["w"], c["h"], c["k"], c["flags"], c["frames"], c["ns"]
        n = len(frames)
        sh = scenes.tilted_shadow_camera() if c["tilted"] else scenes.shadow_camera()
        eye = scenes.eye_camera()
        if c["moved"]:
            eye = dataclasses.replace(eye, position=(-1.0, 0.13, -0.21))
        b0, b1 = c["rows"]
        same_out = c["same_out"] and n > 1
        outs = [torch.full((b1 - b0, w, 4), float("nan"), dtype=torch.float32, device="cuda")
                for _ in range(1 if same_out else n)]
        ptrs = [outs[0].data_ptr()] * n if same_out else [o.data_ptr() for o in outs]
        what = _describe(c)
        ctx.set_lanes(c["lanes"])
        ctx.set_batch(c["batch"])
        torch.cuda.synchronize()
        if c["api"] == "async":
            ctx.render_async(frames[0], eye, sh, w, h, k, flags, ptrs[0])
        elif c["api"] == "rows":
            ctx.render_rows_async(frames[0], eye, sh, w, h, k, flags, rtm.abi.RTM_FORMAT_RGBA32F, ptrs[0], b0, b1)
        else:
            ctx.render_frames_async(frames, eye, sh, w, h, k, flags, ptrs)
        ctx.synchronize()
        assert oob(rtm, ctx) == 0, what
        last_binned = ns[-1] > 16
        assert ctx.last_sphere_path() == int(last_binned), what
        if c["api"] == "frames" and max(ns) > 16:
            assert ctx.last_lanes() == 1 and ctx.last_batch() == 1, what
        binned_frames += sum(m > 16 for m in ns)
        for i in ([n - 1] if same_out else range(n)):
            last = i == n - 1
            want = oracle.render(frames[i], eye, sh, w, h, k, flags, nthreads=NT, want_shadow=last)
            got = (outs[0] if same_out else outs[i]).cpu().numpy()
            assert bits_equal(got, want["rgba"][b0:b1]), f"{what}, frame {i}: {first_mismatch(got, want['rgba'][b0:b1])}"
            # (a fused frame of the kernel-argument path keeps no map; a binned one materialises it)
            if last and (last_binned or not flags & FUSED):
                m = _smap(ctx, w, h)
                assert bits_equal(m, want["shadow"]), f"{what}, last map: {first_mismatch(m, want['shadow'])}"
        if last_binned:
            plan = tuple(int(rtm.bin_plan(frames[-1], cam, w, h)[1].astype(np.int64).sum()) for cam in (eye, sh))
            assert ctx.last_bin_refs() == plan, what
        del outs
    ctx.set_lanes(0)
    ctx.set_batch(0)
    assert binned_frames >= 9 + 4  # (the ring's 4 slots: every one reused at least twice)


_CTX = {}


def _ctx(rtm):
    """ONE context for every chunk of the sequence (state carried across chunks)."""
    if "c" not in _CTX:
        _CTX["c"] = rtm.Context(0)
        assert oob(rtm, _CTX["c"]) >= 0  # (clears the device-wide count)
    return _CTX["c"]
