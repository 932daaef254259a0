"""Cost of the directional / sun / sphere lights' path on the m1 soup: its area light, then a sunlight (4 samples) and a spherelight (1 and
4 samples) in its place.  Same method for all: wall time of yafaray_render after one warm-up render (best of three), rays from
getRenderStats.  usage: python tools/time_lights.py [out.json]  (YAFGPU_VERBOSE=1 prints which shading kernel each scene takes)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libyafaray_amd import Interface, scenes  # noqa: E402

w, sc0, rd = bench.make_workload("m1")
cases = {
    "area": sc0["lights"],
    "sun4": [{"type": "sunlight", "direction": (0.2, -1.0, 0.3), "color": (1.0, 1.0, 1.0), "power": 3.0, "angle": 0.27, "samples": 4}],
    "sphere1": [{"type": "spherelight", "from": (0.0, 0.0, 0.8), "radius": 0.1, "color": (1.0, 1.0, 1.0), "power": 15.0, "samples": 1}],
    "sphere4": [{"type": "spherelight", "from": (0.0, 0.0, 0.8), "radius": 0.1, "color": (1.0, 1.0, 1.0), "power": 15.0, "samples": 4}],
}
out = {}
for name, lights in cases.items():
    yi = Interface()
    scenes.load_scene(yi, dict(sc0, lights=lights), rd)
    yi.render()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); yi.render(); ts.append(time.perf_counter() - t0)
    st = yi.getRenderStats()
    rays = st.rays_closest + st.rays_shadow
    out[name] = {"ms": [round(1e3 * t, 2) for t in ts], "rays": int(rays), "rays_shadow": int(st.rays_shadow),
                 "mrays_per_s_best": round(rays / min(ts) / 1e6, 1)}
    print(name, json.dumps(out[name]), flush=True)
    yi.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
