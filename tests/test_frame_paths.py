"""What a caller can see of the choice between the two sphere paths (csrc/rtm_api.cpp: at
most RTM_MAX_SPHERES spheres as kernel arguments, more through binned device lists) --
frames, the last frame's shadow map and path, the row-range refusal, the refusals of the
calls without a binned path, and the timing history of each of the three enqueue paths.
Pinned so that the entry points can be moved onto one prepare + enqueue without a change
a caller could observe.  65 x 9 (one partial tile column, two tile rows), 8 steps."""
import ctypes as C

import pytest

from conftest import bits_equal, device_smap, first_mismatch

pytestmark = pytest.mark.gpu

W, H, K = 65, 9, 8


@pytest.fixture(scope="module")
def fields(scenes, oracle):
    """A 16- and a 17-sphere field (spheres large enough to cover pixels of a 65 x 9 image,
    different seeds) with their oracle frames and shadow maps, computed once."""
    out = {}
    for n in (16, 17):
        scene = scenes.sphere_field(n, seed=0x2018 + n, rmin=0.05, rmax=0.2)
        ref = oracle.render(scene, scenes.eye_camera(), scenes.shadow_camera(), W, H, K, 0, want_shadow=True)
        ref["rgba"].setflags(write=False)
        ref["shadow"].setflags(write=False)
        out[n] = (scene, ref)
    return out


def test_mixed_sequence(rtm, gpu_ctx, scenes, fields):
    """16, 17, 16 spheres in one rtm_render_frames_async: each frame the oracle's, the
    context's path and shadow map the last frame's."""
    import torch
    order = (16, 17, 16)
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in order]
    torch.cuda.synchronize()
    gpu_ctx.render_frames_async([fields[n][0] for n in order], scenes.eye_camera(), scenes.shadow_camera(), W, H, K, 0,
                                [o.data_ptr() for o in outs])
    gpu_ctx.synchronize()
    for i, n in enumerate(order):
        got, ref = outs[i].cpu().numpy(), fields[n][1]["rgba"]
        assert bits_equal(got, ref), (i, first_mismatch(got, ref))
    for what in ("rgba", "shadow"):  # (the two scenes do differ in both)
        assert not bits_equal(fields[16][1][what], fields[17][1][what]), what
    assert gpu_ctx.last_sphere_path() == 0
    smap = device_smap(gpu_ctx, W, H)
    assert bits_equal(smap, fields[16][1]["shadow"]), first_mismatch(smap, fields[16][1]["shadow"])
    n = C.c_int64(-1)
    assert rtm.load_library().rtm_ctx_oob_reads(gpu_ctx.handle, C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("rows", [(-1, 4), (0, 10), (4, 4)], ids=lambda r: f"{r[0]}_{r[1]}")
def test_row_range_refusal_is_one_message(rtm, gpu_ctx, scenes, fields, rows):
    import torch
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    for n in (16, 17):
        with pytest.raises(rtm.RtmError) as e:
            gpu_ctx.render_rows_async(fields[n][0], scenes.eye_camera(), scenes.shadow_camera(), W, H, K, 0,
                                      rtm.abi.RTM_FORMAT_RGBA32F, out.data_ptr(), rows[0], rows[1])
        assert e.value.code == rtm.abi.RTM_ERR_INVALID, n
        assert f"row range [{rows[0]},{rows[1]}) outside [0,{H})" in str(e.value), (n, str(e.value))


def test_calls_without_a_binned_path(rtm, gpu_ctx, scenes, fields):
    """17 spheres into the stripes and the counters call: -2 (RTM_ERR_UNSUPPORTED)."""
    import torch
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    scene, eye, sh = fields[17][0], scenes.eye_camera(), scenes.shadow_camera()
    with pytest.raises(rtm.RtmError) as e:
        gpu_ctx.render_stripes_async(scene, eye, sh, W, H, K, 0, rtm.abi.RTM_FORMAT_RGBA32F, 4, 2, 0, out.data_ptr())
    assert e.value.code == -2
    with pytest.raises(rtm.RtmError) as e:
        gpu_ctx.stats(scene, eye, sh, W, H, K)
    assert e.value.code == -2


def test_timing_history_of_each_enqueue_path(rtm, scenes, fields):
    """One timed frame through the single-frame, the binned and the batched enqueue: each
    leaves one history entry with a shadow and an eye time."""
    import torch
    eye, sh = scenes.eye_camera(), scenes.shadow_camera()
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    ctx = rtm.Context(0)
    try:
        def single():
            ctx.render_async(fields[16][0], eye, sh, W, H, K, 0, outs[0].data_ptr())

        def binned():
            ctx.render_async(fields[17][0], eye, sh, W, H, K, 0, outs[0].data_ptr())

        def batched():
            ctx.render_frames_async([fields[16][0]] * 2, eye, sh, W, H, K, 0, [o.data_ptr() for o in outs])

        for name, call in (("single", single), ("binned", binned), ("batched", batched)):
            ctx.set_timing_capacity(4)  # (also empties the history)
            call()
            ctx.synchronize()
            if name == "batched":
                assert ctx.last_batch() == 2 and ctx.last_lanes() == 1
            sm, em = ctx.kernel_ms_history(4)
            assert len(sm) == len(em) == 1, (name, sm, em)
            assert sm[0] > 0.0 and em[0] > 0.0, (name, sm, em)
    finally:
        ctx.close()
