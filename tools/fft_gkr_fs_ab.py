#!/usr/bin/env python3
"""fft_gkr with its challenges drawn on the device against fft_gkr on a tape, alternated in one process:
    python tools/fft_gkr_fs_ab.py [REPEATS] [LG ...]          (default: 8 runs at lg = 11 and 17)
vp_fft_gkr_fs from a fixed start state against vp_fft_gkr (batched form, the default) on the tape the first call drew — the same messages, checked — after
two warm-up calls of each; per run the host wall clock of the call and its device time (vp_commit_stats).  The tape form is the floor that non-interactivity
cannot reach: it takes every challenge up front and fuses rounds into launches.  Then one profiled vp_fft_gkr_fs: where the gap goes, from the launch table
(include/vpgpu.h) — the drawing launches, the rounds above the tail, their closing launches, the tails — and the cost of one chain step on one lane, from the
rows that do nothing else.  Prints markdown."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(repeats, sizes):
    sys.path.insert(0, ROOT)
    import numpy as np
    import vp_loader
    vp = vp_loader.load()
    L = vp.lib_gpu()
    vpt, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.vp_get_launch_stats.argtypes = [vpt, ctypes.POINTER(vp.LaunchStat), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.vp_commit_stats.argtypes = [vpt, ctypes.POINTER(ctypes.c_double)]
    L.vp_set_profiling.argtypes = [vpt, ctypes.c_int]
    c = ctypes.c_void_p()
    assert L.vp_create_with_options(0, None, ctypes.byref(c)) == 0
    state = bytes(range(32))

    def dev_ms():
        ms = ctypes.c_double(0)
        assert L.vp_commit_stats(c, ctypes.byref(ms)) == 0
        return ms.value

    for lg in sizes:
        nt, nm = 2 * lg * lg + 9 * lg + 96, 84 + 6 * lg * lg + 8 * lg
        msgs, tape, msgs2 = np.zeros((nm, 2), np.uint64), np.zeros((nt, 2), np.uint64), np.zeros((nm, 2), np.uint64)
        si, so, nw = ctypes.create_string_buffer(state, 32), ctypes.create_string_buffer(32), u64(0)

        def fs():
            t = time.perf_counter()
            assert L.vp_fft_gkr_fs(c, lg, ctypes.cast(si, vpt), msgs.ctypes.data, nm, ctypes.byref(nw), tape.ctypes.data, ctypes.cast(so, vpt)) == 0
            return 1e3 * (time.perf_counter() - t), dev_ms()

        def tp():
            t = time.perf_counter()
            assert L.vp_fft_gkr(c, lg, tape.ctypes.data, nt, msgs2.ctypes.data, nm, ctypes.byref(nw)) == 0
            return 1e3 * (time.perf_counter() - t), dev_ms()

        for _ in range(2):
            fs(); tp()
        assert msgs.tobytes() == msgs2.tobytes(), "the two forms give different messages on the same tape"
        runs = [(fs(), tp()) for _ in range(repeats)]
        steps = nt + nm
        print("## lg = %d: %d chain steps (%d messages absorbed, %d slots drawn), %d alternated runs\n" % (lg, steps, nm, nt, repeats))
        print("| run | vp_fft_gkr_fs: host ms | device ms | vp_fft_gkr on that tape: host ms | device ms |")
        print("|---|---|---|---|---|")
        for i, (a, b) in enumerate(runs):
            print("| %d | %.3f | %.3f | %.3f | %.3f |" % (i, a[0], a[1], b[0], b[1]))
        med = statistics.median
        a_h, a_d, b_h, b_d = ([r[j][k] for r in runs] for j, k in ((0, 0), (0, 1), (1, 0), (1, 1)))
        print("\nmedian host ms: device-drawn %.3f (spread %.3f), tape form %.3f (spread %.3f); gap %.3f ms = %.2f us per chain step"
              % (med(a_h), max(a_h) - min(a_h), med(b_h), max(b_h) - min(b_h), med(a_h) - med(b_h), 1e3 * (med(a_h) - med(b_h)) / steps))
        print("median device ms: device-drawn %.3f, tape form %.3f" % (med(a_d), med(b_d)))
        # one profiled run
        L.vp_set_profiling(c, 1)
        fs()
        n = ctypes.c_int(0)
        arr = (vp.LaunchStat * 1024)()
        assert L.vp_get_launch_stats(c, arr, 1024, ctypes.byref(n)) == 0
        L.vp_set_profiling(c, 0)
        split = {}
        for e in arr[:n.value]:
            k = L.vp_kernel_name(e.kind).decode()
            d = split.setdefault(k, [0, 0.0, 0])
            d[0] += 1; d[1] += e.us; d[2] += e.work if k != "k_round" else 0
        name = {"k_merkle": "drawing launches (k_fg_fs_draw)", "k_round": "rounds above the tail (k_fg_fs_round)",
                "k_emit_multi": "their closing launches (k_fg_fs_close)", "k_seg_multi": "tails (k_fg_fs_tail)"}
        print("\nprofiled run (every new launch bracketed by events; the circuit and table kernels between them are not in the table):\n")
        print("| rows | launches | device us | chain steps in them | us per chain step |")
        print("|---|---|---|---|---|")
        tot = 0.0
        for k in ("k_merkle", "k_round", "k_emit_multi", "k_seg_multi"):
            if k in split:
                cnt, us, work = split[k]
                tot += us
                print("| %s | %d | %.1f | %s | %s |" % (name[k], cnt, us, work if work else "-", "%.2f" % (us / work) if work else "-"))
        print("\n%d launches in the table, %.3f ms in them\n" % (n.value, tot / 1e3))
    L.vp_destroy(c)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if a else 8, a[1:] or [11, 17])
