"""How wf_trace's launches end: reads the exit log of a measurement build (-DYAFGPU_TRACE_EXIT_LOG=1, selected with
YAFARAY_LIBRARY) after a few passes of a bench workload and prints, per busy traversal launch of the last passes, the time from
the first wave's exit to the last, the integral of idle wave slots over that time, and the reservations the waves made.
usage: YAFARAY_LIBRARY=<measurement build> python tools/exit_times.py [workload] [passes]
Times are wall_clock64 ticks of 10 ns (the 100 MHz constant clock)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libyafaray_amd import Interface, interface, scenes  # noqa: E402

TICK_US = 0.01
workload = sys.argv[1] if len(sys.argv) > 1 else "m1"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
busy = int(os.environ.get("EXIT_TIMES_BUSY", 1_000_000))      # launches with at least so many rays are reported

lib = interface.load()
if not hasattr(lib, "yafgpu_exit_log_read"):
    sys.exit("this library is not a measurement build (compile the device unit with -DYAFGPU_TRACE_EXIT_LOG=1)")
lib.yafgpu_exit_log_read.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
lib.yafgpu_exit_log_read.restype = C.c_int

w, sc, rd = bench.make_workload(workload)
yi = Interface()
scenes.load_scene(yi, sc, rd)
yi.setShard(0, 1)
yi.prepareRender()
W, H = yi.getRenderSize()
dev = torch.device("cuda", 0)
planes = torch.zeros((4, H, W, 5), dtype=torch.float32, device=dev)
counters = torch.zeros(8, dtype=torch.int64, device=dev)
stream = torch.cuda.current_stream().cuda_stream
for _ in range(2):
    yi.renderPassDevice(planes.data_ptr(), counters.data_ptr(), stream)
torch.cuda.synchronize()
lib.yafgpu_exit_log_read(None, 0, 1)
for _ in range(passes):
    yi.renderPassDevice(planes.data_ptr(), counters.data_ptr(), stream)
torch.cuda.synchronize()
cap = 1 << 20
buf = np.zeros((cap, 8), np.uint32)
n = lib.yafgpu_exit_log_read(buf.ctypes.data, cap, 1)
if n < 0:
    sys.exit("reading the exit log failed")
a = buf[:min(n, cap)].astype(np.int64)
t_exit, t_start = a[:, 0] | (a[:, 1] << 32), a[:, 2] | (a[:, 3] << 32)
t0 = int(t_start.min()) if len(a) else 0
print(f"{workload}: {passes} passes, {n} wave records")
print("kind     rays      waves  start_us  ramp_us  run_us  spread_us  p50_to_last_us  p10_to_last_us  idle_wave_us  idle_as_machine_us  reservations  per_wave")
launches = []
for kind in (0, 1):
    sel = np.flatnonzero(a[:, 5] == kind)
    sel = sel[np.argsort(t_exit[sel], kind="stable")]
    # one launch: a run of records with the same queue length (consecutive launches of a kind differ in it; between the passes'
    # equal ones the other launches of the pass lie, so the run is also cut where a wave starts after the run's last exit so far)
    runs, cur, cur_last = [], [], 0
    for i in sel:
        if cur and (a[i, 4] != a[cur[0], 4] or t_start[i] > cur_last + 5000):
            runs.append(cur); cur = []
        cur.append(i)
        cur_last = int(t_exit[i])      # (sorted by exit time)
    if cur:
        runs.append(cur)
    for r in runs:
        r = np.asarray(r)
        launches.append((int(t_start[r].min()), kind, r))
for _, kind, r in sorted(launches, key=lambda x: x[0]):
    rays = int(a[r[0], 4])
    if rays < busy:
        continue
    ex, st = t_exit[r], t_start[r]
    last, first = int(ex.max()), int(ex.min())
    idle = float((last - ex).sum()) * TICK_US
    res = int(a[r, 6].sum())
    print(f"{'any' if kind else 'closest':8s} {rays:9d} {len(r):6d} {(int(st.min()) - t0) * TICK_US:9.1f} {(int(st.max()) - int(st.min())) * TICK_US:8.1f} "
          f"{(last - int(st.min())) * TICK_US:7.1f} {(last - first) * TICK_US:10.1f} {(last - float(np.median(ex))) * TICK_US:15.1f} "
          f"{(last - float(np.percentile(ex, 10))) * TICK_US:15.1f} {idle:13.0f} {idle / len(r):19.1f} {res:13d} {res / len(r):9.2f}")
yi.close()
