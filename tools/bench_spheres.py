"""Time the two sphere paths over the scene size: 3840x2160, K = 64, RGBA32F device output,
scenes.sphere_field(n, rmin=0.01 s, rmax=0.08 s) with s = min(1, sqrt(256 / n)) for
n in {16, 17, 256, 4096, 65536}.  n = 16 is the kernel-argument path, everything above
the binned path (device sphere tables + per-tile lists, DESIGN.md "Many spheres").

Per n: distinct frames (one seed each) into a ring of outputs larger than the Infinity
Cache, every frame first checked against the CPU oracle at 256x144, then three
alternating repeats after a warm-up, timed with HIP events on the context's stream.
Reports us per frame, the mean and max list length from bin_plan, and the split between
the shadow pass, the eye pass (rtm_ctx_kernel_ms_history) and the rest of the frame (the
host's table build, the table upload and the list fill together; the kernels among them
are timed by running this tool under `rocprofv3 --kernel-trace --stats`), and checks that
binning beats brute force: t(4096) < 256 x t(16).  Writes one JSON file (--out) and prints it.

Usage: python tools/bench_spheres.py [--out profiles/many_spheres_bench.json]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SIZES = (16, 17, 256, 4096, 65536)


def field(scenes, n, seed):
    if n == 17:
        # the cost of crossing the limit: the n = 16 frame with a 17th sphere off-screen,
        # so both paths render the same image
        sc = field(scenes, 16, seed)
        sc.spherePrimitives.append(scenes.PrimitiveSphere(16, scenes.Shading(0.9, 0.9, 0.2), (0.0, 50.0, 0.5), 0.05))
        return sc
    s = min(1.0, math.sqrt(256.0 / n))
    return scenes.sphere_field(n, seed=seed, rmin=0.01 * s, rmax=0.08 * s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_spheres_bench.json"))
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3, help="distinct frames (and outputs) per n")
    ap.add_argument("--reps", type=int, default=4, help="passes over the frames per timed repeat")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    a = ap.parse_args()
    import numpy as np
    import torch
    import oracle
    rtm = importlib.import_module("2018rustraytracer_amd")
    scenes = importlib.import_module("2018rustraytracer_amd.scenes")
    w, h, k, F = a.width, a.height, a.steps, a.frames
    eye, sh = scenes.eye_camera(), scenes.shadow_camera()
    ctx = rtm.Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream, device="cuda:0")
    outs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(F)]
    ptrs = rtm.Context.out_array([o.data_ptr() for o in outs])
    small = torch.empty((144, 256, 4), dtype=torch.float32, device="cuda:0")
    per_n = {}
    for n in a.sizes:
        fr = [field(scenes, n, 0x2018 + f) for f in range(F)]
        for f, sc in enumerate(fr):  # exact at 256x144 before any timing
            want = oracle.render(sc, eye, sh, 256, 144, k, 0, nthreads=min(16, os.cpu_count() or 1))["rgba"]
            ctx.render_async(sc, eye, sh, 256, 144, k, 0, small.data_ptr())
            ctx.synchronize()
            got = small.cpu().numpy()
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                raise SystemExit(f"n={n} frame {f}: the GPU frame differs from the oracle at 256x144")
        plan = {}
        for name, cam in (("eye", eye), ("shadow", sh)):
            (tw, th), counts = rtm.bin_plan(fr[0], cam, w, h)
            plan[name] = dict(tile=[tw, th], tiles=int(counts.size), mean_list=round(float(counts.mean()), 3),
                              max_list=int(counts.max()), refs=int(counts.sum()))
        per_n[n] = dict(n=n, frames=fr, prepared=ctx.prepare_frames(fr), plan=plan, us=[], wall_us=[], split=[])
    ctx.set_timing_capacity(F)

    def run(n, reps):
        d = per_n[n]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(reps):
            ctx.render_frames_async(None, eye, sh, w, h, k, 0, ptrs, prepared=d["prepared"])
        e1.record(stream)
        e1.synchronize()
        wall = (time.perf_counter() - t0) * 1e6 / (reps * F)
        return e0.elapsed_time(e1) * 1e3 / (reps * F), wall

    for n in a.sizes:  # warm-up: buffers grown, tables built
        run(n, 1)
    for _ in range(3):  # three alternating repeats
        for n in a.sizes:
            us, wall = run(n, a.reps)
            d = per_n[n]
            d["us"].append(round(us, 2))
            d["wall_us"].append(round(wall, 2))
            if ctx.last_sphere_path() == 1:  # one launch per pass per frame: per-frame durations
                sm, em = ctx.kernel_ms_history(F)
                s_us, e_us = 1e3 * sum(sm) / len(sm), 1e3 * sum(em) / len(em)
                d["split"].append(dict(shadow_pass_us=round(s_us, 2), eye_pass_us=round(e_us, 2),
                                       rest_of_frame_us=round(us - s_us - e_us, 2)))
    res = dict(width=w, height=h, steps=k, frames_per_n=F, reps=a.reps,
               ring_bytes=F * w * h * 16, device=torch.cuda.get_device_name(0), sizes=[])
    for n in a.sizes:
        d = per_n[n]
        res["sizes"].append(dict(n=n, path="binned" if n > rtm.abi.RTM_MAX_SPHERES else "kernel arguments",
                                 us_per_frame=d["us"], best_us_per_frame=min(d["us"]), host_wall_us_per_frame=d["wall_us"],
                                 plan=d["plan"], split=d["split"]))
    best = {n: min(per_n[n]["us"]) for n in a.sizes}
    if 16 in best and 4096 in best:
        res["t4096_over_t16"] = round(best[4096] / best[16], 3)
        res["binning_beats_brute_force"] = bool(best[4096] < 256 * best[16])
    if 16 in best and 17 in best:
        res["t17_over_t16"] = round(best[17] / best[16], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    ctx.close()
    if res.get("binning_beats_brute_force") is False:
        raise SystemExit("n = 4096 took more than 256 x the n = 16 frame")


if __name__ == "__main__":
    main()
