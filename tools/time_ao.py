"""Cost of ambient occlusion on the m1 soup's geometry under the direct lighting integrator: AO off, AO_samples 8 and AO_samples 32.
Same method as tools/time_lights.py: wall time of yafaray_render after one warm-up render (best of three), rays from getRenderStats.
usage: python tools/time_ao.py [out.json]  (YAFGPU_VERBOSE=1 prints which shading kernel each case takes: the specialised one without AO,
the general one with it)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from libyafaray_amd import Interface, scenes  # noqa: E402

w, sc, rd0 = bench.make_workload("m1")
rd0 = dict(rd0, integrator="directlighting")
cases = {
    "off": {},
    "ao8": {"do_AO": True, "AO_samples": 8, "AO_distance": 0.3},
    "ao32": {"do_AO": True, "AO_samples": 32, "AO_distance": 0.3},
}
out = {}
for name, ao in cases.items():
    yi = Interface()
    scenes.load_scene(yi, sc, dict(rd0, **ao))
    yi.render()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); yi.render(); ts.append(time.perf_counter() - t0)
    st = yi.getRenderStats()
    rays = st.rays_closest + st.rays_shadow
    out[name] = {"ms": [round(1e3 * t, 2) for t in ts], "camera_samples": int(st.camera_samples), "rays": int(rays), "rays_shadow": int(st.rays_shadow),
                 "mrays_per_s_best": round(rays / min(ts) / 1e6, 1)}
    print(name, json.dumps(out[name]), flush=True)
    yi.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
