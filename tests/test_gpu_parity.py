"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs."""
import numpy as np
import pytest

from libyafaray_amd import Interface, interface, scenes
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

DEVICE_TREE = __import__("os").environ.get("YAFGPU_BUILD") == "device"     # the suite also runs with the GPU-built tree
RTOL = 1e-4     # BASELINE.json north_star: per-pixel RGB within 1e-4 relative
ABS_FLOOR = 1e-3


def compare_films(gpu_film, ora_film, what, max_outliers=0, exact_weights=True):
    a, b = po.film_to_rgb(gpu_film), po.film_to_rgb(ora_film)
    if exact_weights:
        assert np.array_equal(gpu_film[..., 4], ora_film[..., 4]), f"{what}: film weights differ"
    else:
        np.testing.assert_allclose(gpu_film[..., 4], ora_film[..., 4], rtol=2e-6, err_msg=f"{what}: film weights differ")
    rel = np.abs(a[..., :3] - b[..., :3]) / np.maximum(np.abs(b[..., :3]), ABS_FLOOR)
    worst = rel.max(axis=-1)
    n_bad = int((worst > RTOL).sum())
    exact = float((gpu_film == ora_film).all(axis=-1).mean())
    print(f"{what}: {n_bad}/{worst.size} pixels over {RTOL}, max rel {worst.max():.3g}, bit-exact pixels {exact:.4f}")
    if exact_weights:   # alpha sums round like the colour sums (plane order, see DESIGN.md "film"): the last bit may differ
        assert np.allclose(a[..., 3], b[..., 3], rtol=1e-6, atol=1e-7), f"{what}: alpha differs"
    assert n_bad <= max_outliers, f"{what}: {n_bad} pixels over tolerance (max rel {worst.max():.3g})"
    return n_bad, exact


@pytest.fixture(params=["wavefront"], autouse=True)
def pipeline(request):
    """The one pipeline there is.  (A parameter of every test of this module, so that their ids stay those the suite's records name.)"""
    return request.param


def render_both(sc, rd):
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film = yi.getFilm(rd["width"], rd["height"])
    st = yi.getRenderStats()
    osc = po.OracleScene(sc)
    ofilm, ost = osc.render(rd)
    return film, st, ofilm, ost


def test_ray_batches_match_oracle():
    sc = scenes.cornell_soup(3000, seed=11)
    yi = Interface()
    scenes.load_scene(yi, sc, scenes.render_settings(32, 32, 1))
    yi.prepareRender()
    osc = po.OracleScene(sc)
    rng = np.random.default_rng(5)
    n = 20000
    o = rng.uniform(-0.95, 0.95, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d.astype(np.float32), np.full((n, 1), 5e-5, np.float32), np.full((n, 1), -1.0, np.float32)], axis=1)
    rays[::7, 7] = rng.uniform(0.05, 1.0, size=rays[::7].shape[0])   # bounded rays too
    tri, t, bary = yi.intersectRays(rays)
    sh = yi.shadowRays(rays)
    mism = 0
    for i in range(n):
        h, oti, ot, ob = osc.intersect(rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7]), use_tree=False)
        if (tri[i] >= 0) != bool(h) or (h and (tri[i] != oti or t[i] != ot or not np.array_equal(bary[i], ob))):
            mism += 1
        s = osc.is_shadowed(rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7]), use_tree=False)
        if bool(s) != bool(sh[i]):
            mism += 1
    assert mism == 0, f"{mism} ray results differ from the brute-force oracle"


@pytest.mark.parametrize("n_tris,res,spp,bounces", [(12, 32, 4, 2), (500, 48, 16, 3), (5000, 64, 16, 3), (2000, 40, 64, 2), (800, 33, 3, 4)])
def test_render_matches_oracle(n_tris, res, spp, bounces):
    sc = scenes.cornell_soup(n_tris, seed=n_tris, res=(res, res))
    rd = scenes.render_settings(res, res, spp, bounces=bounces)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.camera_samples == res * res * spp
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow, "ray counts differ from the oracle"
    compare_films(film, ofilm, f"cornell {n_tris} tris {res}x{res} {spp}spp b{bounces}")


@pytest.mark.parametrize("rr_min", [3, 1])
def test_per_sample_streams_match_the_oracle(rr_min):
    """Serial-state replay off, two lights: estimateOneDirectLight's counter starts every camera sample at its ordinal x 16
    (st_after_closest) and Russian roulette draws from the sample's own MWC stream (st_start_path).  The oracle restates
    that mode (per_sample_streams).  rr_min 3: roulette off, the counter alone; rr_min 1: roulette from depth 1 on too."""
    sc = scenes.cornell_soup(3000, seed=77, res=(56, 40), n_lights=2, glossy_fraction=0.3)
    rd = scenes.render_settings(56, 40, 12, bounces=3, path_samples=2, russian_roulette_min_bounces=rr_min)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setSerialReplay(False)
    yi.render()
    film, st = yi.getFilm(56, 40), yi.getRenderStats()
    ofilm, ost = po.OracleScene(sc).render(dict(rd, per_sample_streams=True))
    assert st.camera_samples == ost.camera_samples == 56 * 40 * 12
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow, "ray counts differ from the oracle"
    compare_films(film, ofilm, f"per-sample streams, roulette from depth {rr_min}")


def test_glossy_two_lights_point_light_run_and_match_oracle_where_defined():
    """Glossy (as_diffuse) + diffuse, ONE area light: inside the deterministic-parity regime."""
    sc = scenes.cornell_soup(1500, seed=5, res=(40, 40), glossy_fraction=0.5)
    rd = scenes.render_settings(40, 40, 16, bounces=3)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "glossy 50% cornell")
    # a point light (Dirac branch of doLightEstimation) in place of the area light
    sc2 = scenes.cornell_soup(800, seed=6, res=(32, 32))
    sc2["lights"] = [{"type": "pointlight", "from": (0.2, -0.3, 0.6), "color": (1.0, 0.9, 0.8), "power": 3.0}]
    rd2 = scenes.render_settings(32, 32, 8, bounces=2)
    film, st, ofilm, ost = render_both(sc2, rd2)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "point light cornell")


def test_config0_test01_xml_path_tracing():
    """BASELINE.json config 0: the reference's own test scene (tests/test01/test01.xml, textures removed,
    integrator switched to pathtracing per SURVEY Appendix C), 256x256, 16 spp — loaded by the C++ XML
    loader, rendered on the GPU, compared with the oracle fed by an independent Python parse of the same file."""
    import os
    from tests import xml_scene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test01_pt.xml")
    yi = Interface()
    yi.loadXml(path)
    yi.render()
    film = yi.getFilm(256, 256)
    st = yi.getRenderStats()
    sc, rd = xml_scene.load(path)
    ofilm, ost = po.OracleScene(sc).render(dict(rd, oracle_threads=8))
    assert st.n_triangles == 74 and st.camera_samples == 256 * 256 * 16
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "test01 path tracing 256x256 16spp")


def test_test01_xml_shipped_settings_direct_lighting_gauss():
    """The reference's test scene with the integrator and film settings it ships (tests/test01/test01.xml:
    directlighting, 480x270, 1 spp, gauss 1.5 — the render behind BASELINE.md's 0.9 s badge), textures removed."""
    import os
    from tests import xml_scene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test01_dl.xml")
    yi = Interface()
    yi.loadXml(path)
    yi.render()
    film = yi.getFilm(480, 270)
    st = yi.getRenderStats()
    sc, rd = xml_scene.load(path)
    ofilm, ost = po.OracleScene(sc).render(dict(rd, oracle_threads=8))
    assert st.camera_samples == 480 * 270
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "test01 shipped settings", exact_weights=False)


def test_device_whole_path_against_the_references_expected_png():
    """The DEVICE render of the reference's shipped test scene (textures stripped) through the reference's output
    transform, against the expected PNG the reference's tests hold — every pixel whose filter footprint sees only
    untextured materials (47 % of the frame; tests/png_fixture.py).  The same bounds as the oracle's own check
    (tests/test_oracle_golden.py): >= 99.5 % within two 8-bit levels, >= 96 % within one, >= 80 % equal."""
    import os
    from tests import png_fixture, xml_scene
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test01_dl.xml")
    yi = Interface()
    yi.loadXml(path)
    yi.render()
    film = yi.getFilm(480, 270)
    sc, rd = xml_scene.load(path)
    st = png_fixture.compare(film, sc, rd, "device")
    assert st["fraction_of_frame"] > 0.45
    assert st["within_2"] >= 0.995 * st["pixels_compared"], st
    assert st["within_1"] >= 0.96 * st["pixels_compared"], st
    assert st["exact"] >= 0.80 * st["pixels_compared"], st


def _sphere_soup(n_lat=10, n_lon=16, radius=0.45, centre=(0.0, 0.1, -0.3)):
    """a tessellated sphere with exported vertex normals (addNormal path, Triangle::getSurface smooth branch)"""
    c = np.array(centre, np.float32)
    verts, norms = [], []
    def pt(i, j):
        th = np.pi * i / n_lat; ph = 2 * np.pi * j / n_lon
        n = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], np.float32)
        return c + radius * n, n
    for i in range(n_lat):
        for j in range(n_lon):
            p00, n00 = pt(i, j); p01, n01 = pt(i, j + 1); p10, n10 = pt(i + 1, j); p11, n11 = pt(i + 1, j + 1)
            if i > 0:
                verts.append([p00, p10, p01]); norms.append([n00, n10, n01])
            if i < n_lat - 1:
                verts.append([p01, p10, p11]); norms.append([n01, n10, n11])
    return np.array(verts, np.float32), np.array(norms, np.float32)


def test_vertex_normals_crop_window_sampling_offset_and_alpha():
    sc = scenes.cornell_soup(12, seed=2, res=(64, 48))
    sv, sn = _sphere_soup()
    walls = sc["verts"]
    sc["verts"] = np.concatenate([walls, sv], axis=0)
    sc["vnormals"] = np.concatenate([np.zeros_like(walls), sn], axis=0)      # zero triple = geometric normal
    sc["tri_mat"] = np.concatenate([sc["tri_mat"], np.full(sv.shape[0], 1, np.int32)])
    # crop window, non-zero base sampling offset + computer node, transparent background
    rd = scenes.render_settings(40, 30, 8, bounces=3, xstart=13, ystart=9, adv_base_sampling_offset=7, adv_computer_node=2,
                                bg_transp=True, tile_size=16)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "smooth sphere, crop window, sampling offset, bg_transp")


def test_material_flags_translucency_orennayar_and_direct_lighting():
    sc = scenes.cornell_soup(1200, seed=31, res=(48, 48))
    sc["materials"][0] = {"type": "shinydiffusemat", "color": (0.8, 0.8, 0.7), "diffuse_reflect": 0.9, "diffuse_brdf": "oren_nayar", "sigma": 0.3}
    sc["materials"][1] = {"type": "shinydiffusemat", "color": (0.7, 0.2, 0.2), "diffuse_reflect": 0.8, "translucency": 0.4, "emit": 0.05}
    sc["materials"][2] = {"type": "shinydiffusemat", "color": (0.2, 0.7, 0.2), "visibility": "no_shadows", "receive_shadows": False}
    sc["materials"][4] = {"type": "shinydiffusemat", "color": (0.5, 0.5, 0.9), "visibility": "shadow_only", "flat_material": True}
    sc["tri_mat"][20::9] = 4
    for integ in ("pathtracing", "directlighting"):
        rd = scenes.render_settings(48, 48, 8, bounces=3, integrator=integ, background=(0.05, 0.06, 0.08))
        film, st, ofilm, ost = render_both(sc, rd)
        assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
        compare_films(film, ofilm, f"material flags / translucency / oren-nayar ({integ})")


def test_path_samples_and_deep_bounces():
    sc = scenes.cornell_soup(700, seed=44, res=(32, 32), open_front=False)
    rd = scenes.render_settings(32, 32, 4, bounces=6, path_samples=3)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "closed box, path_samples 3, 6 bounces")


def test_empty_scene_and_single_pixel():
    sc = scenes.cornell_soup(12, seed=1, res=(8, 8))
    sc["verts"] = sc["verts"][:0]; sc["tri_mat"] = sc["tri_mat"][:0]
    rd = scenes.render_settings(8, 8, 2, background=(0.25, 0.5, 0.75))
    film, st, ofilm, ost = render_both(sc, rd)
    assert np.array_equal(film, ofilm) and np.allclose(po.film_to_rgb(film)[..., :3], (0.25, 0.5, 0.75))
    sc = scenes.cornell_soup(50, seed=1, res=(1, 1))
    rd = scenes.render_settings(1, 1, 130)       # one pixel, more samples than a wave, not a multiple of 64
    film, st, ofilm, ost = render_both(sc, rd)
    compare_films(film, ofilm, "1x1 pixel, 130 spp")


@pytest.mark.parametrize("filt,width", [("gauss", 1.5), ("mitchell", 1.2), ("lanczos", 2.0), ("box", 2.5)])
def test_reconstruction_filters(filt, width):
    """ImageFilm's filter table and footprint (imagefilm.cc:124-187, 925-1015) beyond the 1-pixel box: the
    reference's own test scene ships with gauss 1.5.  Neighbour splats go through float atomics, so the sum
    order — and only that — differs from the oracle: same tolerance, weights to 2e-6."""
    sc = scenes.cornell_soup(900, seed=12, res=(45, 37))
    rd = scenes.render_settings(45, 37, 6, bounces=2, filter_type=filt, AA_pixelwidth=width, background=(0.1, 0.1, 0.2))
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"{filt} {width}", exact_weights=False)


# ---- BASELINE.json's full-size configurations -----------------------------------------------------------
# In the parity regime the film is a pure function of (pixel, sample index) (experiment 2), so the
# oracle rendering a CROP WINDOW of the frame must reproduce that region of the full-size GPU film — except the
# crop's first row and column, which in the full frame also receive the box filter's splats from the pixels
# above / to the left (ImageFilm::addSample).  That pins the full-size renders to the oracle at a cost of a few
# tens of thousands of oracle samples per window.
def _oracle_threads():
    import bench
    return max(1, min(32, bench.host_cpu_share()))


def _full_size_against_crops(name, crops, size, lights=None, low_spp=4):
    """(1) the configuration at its full size on the GPU, pinned to the oracle on crop windows that together cover
    >= 5 % of the frame; (2) the WHOLE frame at `low_spp` samples per pixel against the oracle's whole frame — in the
    parity regime the film is a pure function of (pixel, sample index), so every pixel of the full-size frame is
    checked at its first samples, at the full triangle count (where a traversal leak or a tie would show)."""
    import bench
    w, sc, rd = bench.make_workload(name, lights=lights)
    W, H = rd["width"], rd["height"]
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film = yi.getFilm(W, H)
    st = yi.getRenderStats()
    assert st.camera_samples == W * H * rd["AA_minsamples"]
    assert st.n_triangles == len(sc["verts"])
    # every sample adds weight 1 to its own pixel, and to the right / lower neighbour as well when its offset is
    # >= 0.999 of a pixel (box half-width 0.501): about 0.1 % of the samples per axis
    n_samples = W * H * rd["AA_minsamples"]
    extra = float(film[..., 4].astype(np.float64).sum()) - n_samples
    assert 0 <= extra < 0.004 * n_samples, f"film weight {extra} over the sample count"
    yi.render()                                   # determinism: the second pass gives the same bits
    assert np.array_equal(film, yi.getFilm(W, H)), "two passes over the same scene differ"
    osc = po.OracleScene(sc)
    threads = _oracle_threads()
    bad = total = 0
    for (x0, y0) in crops:
        ofilm, _ = osc.render(dict(rd, xstart=x0, ystart=y0, width=size, height=size, oracle_threads=threads))
        g = film[y0 + 1:y0 + size, x0 + 1:x0 + size]
        n_bad, exact = compare_films(g, ofilm[1:, 1:], f"{name} full size, window at ({x0},{y0})", max_outliers=max(2, size * size // 2000))
        bad += n_bad; total += g.shape[0] * g.shape[1]
    assert total >= 0.05 * W * H, f"windows cover {total / (W * H):.3f} of the frame"
    assert bad <= max(1, total // 2000)       # two builds of the reference itself differ on ~3e-5 of pixels
    # whole frame, few samples
    rd_low = dict(rd, AA_minsamples=low_spp)
    yi2 = Interface()
    scenes.load_scene(yi2, sc, rd_low)
    yi2.render()
    film_low, st_low = yi2.getFilm(W, H), yi2.getRenderStats()
    ofilm, ost = osc.render(dict(rd_low, oracle_threads=threads))
    osc.close()
    assert st_low.rays_closest == ost.rays_closest and st_low.rays_shadow == ost.rays_shadow, f"{name} whole frame at {low_spp} spp: ray counts differ"
    compare_films(film_low, ofilm, f"{name} WHOLE frame {W}x{H} at {low_spp} spp", max_outliers=max(1, W * H // 20000))
    return st


def test_full_size_m1_against_oracle_windows():
    """The configuration BASELINE.json's metric is quoted on (bench.py's default): 1M triangles, 512x512, 64 spp,
    primary + 1 bounce.  4 windows of 64x64 = 6 % of the frame at 64 spp + the whole frame at 4 spp."""
    _full_size_against_crops("m1", [(30, 40), (224, 224), (440, 300), (200, 440)], 64)


def test_full_size_c2_against_oracle_windows():
    """BASELINE.json configs[1]: 100k triangles, 512x512, 64 spp, primary + 1 bounce."""
    _full_size_against_crops("c2", [(40, 60), (224, 224), (440, 300), (200, 440)], 64)


def test_full_size_c3_against_oracle_windows():
    """BASELINE.json configs[2]: 1M triangles, 1024x1024, 256 spp, 2 bounces.  4 windows of 116x116 = 5.1 % of the
    frame at 256 spp + the whole frame at 2 spp."""
    _full_size_against_crops("c3", [(100, 700), (454, 454), (800, 200), (600, 880)], 116, low_spp=2)


def test_full_size_c4_one_light_against_oracle_windows():
    """BASELINE.json configs[3] in its one-light variant: 1M triangles, half of them glossy, 1024x1024, 64 spp,
    2 bounces, MIS.  (The two-light configuration as stated: test_full_size_c4_two_lights_exact_replay.)"""
    _full_size_against_crops("c4", [(300, 800), (640, 400), (60, 100), (850, 850)], 116, lights=1, low_spp=2)


# ---- serial-state replay: the reference's per-tile roulette stream and its light counter -------------
@pytest.mark.parametrize("aa", [dict(AA_threshold=0.02), dict(AA_threshold=0.03, AA_detect_color_noise=True, AA_dark_detection_type="linear", AA_dark_threshold_factor=0.6),
                                dict(AA_threshold=0.5, AA_dark_detection_type="curve", AA_variance_pixels=3, AA_variance_edge_size=8)])
def test_noise_detection_on_the_device_equals_the_host_version(aa, monkeypatch):
    """ImageFilm::nextPass's detection (imagefilm.cc:270-480) runs on the device between adaptive passes; the host restatement it
    replaced (YAFGPU_AA_DETECT=host) must flag the same pixels: same resampled counts per pass, same film."""
    sc = scenes.cornell_soup(2000, seed=17, res=(71, 53))
    rd = scenes.render_settings(71, 53, 2, bounces=2, AA_passes=4, AA_inc_samples=2, **aa)
    out = []
    for mode in ("device", "host"):
        monkeypatch.setenv("YAFGPU_AA_DETECT", mode)
        yi = Interface()
        scenes.load_scene(yi, sc, rd)
        yi.render()
        out.append((yi.getFilm(71, 53), yi.getRenderStats().camera_samples))
    assert out[0][1] == out[1][1] and out[0][1] > 71 * 53 * 2, "other pixels were flagged (or none at all)"
    assert np.array_equal(out[0][0], out[1][0])


def test_prepare_render_keeps_the_device_scene_until_something_changes():
    """Scene::update rebuilds the tree only when the scene changed (scene.cc:784-790): a second render() of an untouched scene reuses
    the device scene (no second tree build), a render parameter alone (samples) does not rebuild either, a new camera or a changed
    material does — and the film is then the one a fresh Interface renders."""
    sc = scenes.cornell_soup(3000, seed=3, res=(40, 32))
    rd = scenes.render_settings(40, 32, 2, bounces=2)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    f0, built0 = yi.getFilm(40, 32), yi.getRenderStats().tree_build_seconds
    assert built0 > 0.0
    yi.render()
    assert np.array_equal(yi.getFilm(40, 32), f0)
    assert yi.getRenderStats().tree_build_seconds == built0, "the tree was built again for an unchanged scene"
    # a new camera under the same name: the scene is prepared again and the film is a fresh render's
    cam2 = dict(sc["camera"], **{"from": (0.3, -3.2, 0.2)})
    yi.paramsClearAll(); yi.paramsSet(dict(cam2, type="perspective")); yi.createCamera("cam")
    scenes.set_render_params(yi, rd)
    yi.render()
    f1 = yi.getFilm(40, 32)
    y2 = Interface()
    scenes.load_scene(y2, dict(sc, camera=cam2), rd)
    y2.render()
    assert not np.array_equal(f1, f0) and np.array_equal(f1, y2.getFilm(40, 32))


def _render_with_rand_state(sc, rd, replay=True, same_tree=False):
    """device render + the oracle's SINGLE-THREADED render of the same scene with the libc state the device side derived
    for it (srand seed of the last constructor, values its colour loop consumed): the reference's serial semantics.
    same_tree: the oracle walks the product's kd-tree — multi-pass renders put sample 1 of every pixel on the pixel's
    diagonal (riVdC(1, r) = riS(1, r)), where a camera ray can run exactly into the edge two walls of the box share: a
    tie in t that TriKdTree::intersect resolves by visiting order, i.e. by tree topology (see test_multi_pass_anti_aliasing).
    With serial state one such sample shifts the light counter of every sample after it."""
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setSerialReplay(replay)
    seed, skip = yi.getRandState()
    assert seed > 0 and skip >= 3
    yi.render()
    film, st = yi.getFilm(rd["width"], rd["height"]), yi.getRenderStats()
    osc = po.OracleScene(sc)
    if same_tree:
        osc.set_tree(*interface.build_kdtree(sc["verts"], threads=4, device=DEVICE_TREE)[:3])
    ofilm, ost = osc.render(dict(rd, oracle_threads=1, rand_srand=seed, rand_skip=skip))
    return film, st, ofilm, ost


@pytest.mark.parametrize("case", [
    dict(n_lights=1, bounces=4, rr=0, path_samples=1),                 # the reference's default: roulette from depth 1 on
    dict(n_lights=1, bounces=6, rr=2, path_samples=3),
    dict(n_lights=2, bounces=3, rr=3, path_samples=1),                 # roulette off, two lights: the counter alone
    dict(n_lights=2, bounces=5, rr=0, path_samples=2, glossy=0.4),     # both, MIS on glossy
    dict(n_lights=2, bounces=4, rr=1, path_samples=1, aa=dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02)),   # adaptive passes
    dict(n_lights=1, bounces=4, rr=1, path_samples=1, aa=dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02)),   # ... the stream alone
    dict(n_lights=2, bounces=4, rr=4, path_samples=1, aa=dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02)),   # ... the counter alone
    dict(n_lights=2, bounces=4, rr=1, path_samples=1, aa=dict(AA_passes=2, AA_inc_samples=2, AA_threshold=0.0)),    # every pixel again
    dict(n_lights=2, bounces=4, rr=1, path_samples=1, aa=dict(AA_passes=2, AA_inc_samples=2, AA_threshold=10.0)),   # no pixel again: pass 0 in the multi-pass mode
    # with recursiveRaytrace a camera sample is a tree of integrate() calls: its events are kept per call, in the reference's depth-first order
    dict(n_lights=2, bounces=3, rr=0, path_samples=1, raydepth=2, spec=True),
    dict(n_lights=1, bounces=4, rr=1, path_samples=2, raydepth=3, spec=True),
    dict(n_lights=2, bounces=3, rr=1, path_samples=2, raydepth=2, spec=True, glossy=0.3, glossy_rec=True),      # the glossy branch: 8 trajectories, split path samples
    dict(n_lights=2, bounces=3, rr=0, path_samples=1, raydepth=2, spec=True, aa=dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02)),
])
def test_serial_state_replay_matches_the_single_threaded_oracle(case, monkeypatch):
    """Russian roulette ON (the reference's default, integrator_path_tracer.cc:355) and / or more than one light: the
    film depends on state that runs through the samples in the reference's order — the tile's MWC stream
    (integrator_tiled.cc:319, seeded from libc rand()) and correlative_sample_number_ (integrator_montecarlo.cc:62-76).
    The device replays both (record pass, per-tile scan, final pass) and must reproduce the oracle's one-thread render:
    same ray counts, same film."""
    sc = scenes.cornell_soup(1500, seed=41 + case["bounces"], res=(72, 56), n_lights=case["n_lights"], glossy_fraction=case.get("glossy", 0.0))
    if case.get("spec"):
        m = sc["materials"]
        m[1] = {"type": "shinydiffusemat", "color": (0.8, 0.3, 0.3), "diffuse_reflect": 0.6, "specular_reflect": 0.35, "transparency": 0.25, "transmit_filter": 0.8}
        m[2] = {"type": "glass", "IOR": 1.45, "filter_color": (0.8, 1.0, 0.8), "transmit_filter": 0.6, "mirror_color": (1.0, 1.0, 1.0)}
        if case.get("glossy_rec"):
            m[4] = dict(m[4], as_diffuse=False)
    rd = scenes.render_settings(72, 56, 6, bounces=case["bounces"], path_samples=case["path_samples"], tile_size=16,
                                russian_roulette_min_bounces=case["rr"], **({"raydepth": case["raydepth"]} if "raydepth" in case else {}), **case.get("aa", {}))
    multi = "aa" in case
    film, st, ofilm, ost = _render_with_rand_state(sc, rd, same_tree=multi)
    wdiff = int((film[..., 4] != ofilm[..., 4]).sum())
    exact = float((film == ofilm).all(axis=-1).mean())
    print(f"serial replay {case}: rays {st.rays_closest}+{st.rays_shadow} vs oracle {ost.rays_closest}+{ost.rays_shadow}, samples {st.camera_samples} vs {ost.camera_samples}, "
          f"pixels with another weight {wdiff}, bit-exact pixels {exact:.4f}")
    assert st.camera_samples == ost.camera_samples
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow, "ray counts differ from the oracle's single-thread render"
    compare_films(film, ofilm, f"serial replay {case}")
    # chunk borders (whole tiles per chunk) do not change anything.  (Every scene set-up moves the libc state on — the
    # material counter is process-wide, as in the reference — so each render is compared with its own oracle run.)
    monkeypatch.setenv("YAFGPU_WF_CHUNK", "4096")
    film2, st2, ofilm2, ost2 = _render_with_rand_state(sc, rd, same_tree=multi)
    assert st2.rays_closest == ost2.rays_closest and st2.rays_shadow == ost2.rays_shadow, "chunked replay: ray counts differ from the oracle"
    compare_films(film2, ofilm2, f"serial replay, chunked {case}")
    monkeypatch.delenv("YAFGPU_WF_CHUNK")
    # and the per-sample streams (replay off) render something else: the state does matter in this scene
    film3, st3, _, _ = _render_with_rand_state(sc, rd, replay=False, same_tree=multi)
    assert not np.array_equal(film3, film)


def test_full_size_c4_two_lights_exact_replay():
    """BASELINE.json configs[3] AS STATED — 1M triangles, half of them glossy, TWO area lights, 1024x1024 — whole frame
    at 2 spp against the oracle's single-threaded render (with two lights the light a path vertex samples depends on
    the number of estimateOneDirectLight calls before it in the whole frame, so windows cannot stand in for the frame)."""
    import bench
    w, sc, rd = bench.make_workload("c4", spp=2)
    film, st, ofilm, ost = _render_with_rand_state(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "c4 two lights 1024x1024 2 spp, exact replay", max_outliers=1024 * 1024 // 20000)


def test_device_shards_sum_to_the_unsharded_frame():
    """The multi-GPU decomposition on ONE GPU: shard 0/2 and 1/2 (tile t -> rank t % 2, yafaray_setShard) rendered by the
    device one after the other, their films summed as parallel.reduce_film sums them over RCCL — equal to the unsharded
    device film bit for bit on every pixel that is not on a tile's first row / column (those also take a neighbouring
    tile's box-filter splat, i.e. one addition in another order), and to 1 ulp there."""
    W, H, T = 160, 128, 32
    sc = scenes.cornell_soup(6000, seed=23, res=(W, H), glossy_fraction=0.3)
    rd = scenes.render_settings(W, H, 16, bounces=3, tile_size=T)
    def render(index, count):
        yi = Interface()
        scenes.load_scene(yi, sc, rd)
        yi.setShard(index, count)
        yi.render()
        return yi.getFilm(W, H), yi.getRenderStats()
    full, st_full = render(0, 1)
    for world in (2, 3):
        parts = [render(r, world) for r in range(world)]
        assert sum(p[1].camera_samples for p in parts) == st_full.camera_samples
        assert sum(p[1].rays_closest for p in parts) == st_full.rays_closest and sum(p[1].rays_shadow for p in parts) == st_full.rays_shadow
        total = np.zeros_like(full)
        for f, _ in parts:
            total = total + f
        # ownership: a shard's own-pixel weight is zero outside its tiles (up to border splats)
        ntx = (W + T - 1) // T
        for r, (f, _) in enumerate(parts):
            for t in range(ntx * ((H + T - 1) // T)):
                if t % world != r:
                    tx, ty = t % ntx, t // ntx
                    assert not f[ty * T + 1:(ty + 1) * T, tx * T + 1:(tx + 1) * T, 4].any(), "a shard rendered a tile it does not own"
        interior = np.ones((H, W), bool)
        interior[::T, :] = False; interior[:, ::T] = False
        assert np.array_equal(total[interior], full[interior]), f"{world} shards: interior pixels differ from the unsharded frame"
        assert np.array_equal(total[..., 4], full[..., 4]), "weights differ"
        np.testing.assert_allclose(total, full, rtol=2.5e-7, atol=1e-7)


# ---- multi-pass anti-aliasing: TiledIntegrator::render's pass schedule + ImageFilm::nextPass ----------------
@pytest.mark.parametrize("aa", [
    dict(AA_passes=3, AA_inc_samples=3, AA_threshold=0.0),                                    # every pixel, every pass
    dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.02),                                   # adaptive
    dict(AA_passes=4, AA_inc_samples=2, AA_threshold=0.01, AA_sample_multiplier_factor=1.5,
         AA_light_sample_multiplier_factor=2.0, AA_detect_color_noise=True, AA_dark_detection_type="linear",
         AA_dark_threshold_factor=0.5, AA_variance_edge_size=6, AA_variance_pixels=3, AA_resampled_floor=60.0),
    dict(AA_passes=2, AA_inc_samples=4, AA_threshold=0.005, AA_dark_detection_type="curve", AA_clamp_samples=0.6),
])
def test_multi_pass_anti_aliasing(aa):
    """integrator_tiled.cc:116-258 (pass schedule, sample / light multipliers, threshold decay under the resampled
    floor), :394-398 (riVdC / riS sub-pixel positions), imagefilm.cc:270-480 (noise detection), :975 (sample clamp).
    The set of resampled pixels shows in the film weights, which must match the oracle's exactly."""
    from libyafaray_amd import interface
    sc = scenes.cornell_soup(700, seed=21, res=(56, 44))
    rd = scenes.render_settings(56, 44, 3, bounces=2, background=(0.05, 0.1, 0.2), **aa)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film, st = yi.getFilm(56, 44), yi.getRenderStats()
    # riVdC(1, r) == riS(1, r): sample 1 of every pixel sits on the pixel's diagonal, and in this symmetric box such a
    # camera ray can run exactly into the edge two walls share — an exact tie in t between two triangles of different
    # materials, which TriKdTree::intersect resolves by visiting order (kdtree_triangle.cc:782), i.e. by tree
    # topology.  The oracle therefore walks the same tree as the device here; everywhere else it builds its own.
    osc = po.OracleScene(sc)
    osc.set_tree(*interface.build_kdtree(sc["verts"], threads=4, device=DEVICE_TREE)[:3])
    ofilm, ost = osc.render(rd)
    assert st.camera_samples == ost.camera_samples
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    assert film[..., 4].min() >= 3 and len(np.unique(np.round(film[..., 4]))) >= (1 if aa["AA_threshold"] == 0.0 else 2)
    compare_films(film, ofilm, f"multi-pass {aa}")


@pytest.mark.parametrize("bokeh", [dict(bokeh_type="disk1"), dict(bokeh_type="hexagon", bokeh_bias="edge", bokeh_rotation=20.0),
                                   dict(bokeh_type="ring"), dict(bokeh_type="disk2", bokeh_bias="center")])
def test_depth_of_field(bokeh):
    """aperture != 0: per-pixel Halton(3) / Halton(5) lens coordinates (integrator_tiled.cc:382-383,405-409) through
    PerspectiveCamera::getLensUv (camera_perspective.cc:91-131)"""
    sc = scenes.cornell_soup(600, seed=8, res=(52, 40))
    sc["camera"] = dict(sc["camera"], aperture=0.08, dof_distance=3.7, **bokeh)
    rd = scenes.render_settings(52, 40, 9, bounces=2, background=(0.1, 0.1, 0.1), adv_base_sampling_offset=5)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"depth of field {bokeh}")
    pin = dict(sc); pin["camera"] = dict(sc["camera"], aperture=0.0)
    pfilm, _ = po.OracleScene(pin).render(rd)
    assert not np.allclose(po.film_to_rgb(pfilm), po.film_to_rgb(ofilm), rtol=1e-3), "the lens changes the image"


@pytest.mark.parametrize("angle", [181.0, 40.0])
def test_smooth_mesh_render(angle):
    """Interface::smoothMesh (scene.cc:383-543): vertex normals computed on the host from the shared-vertex mesh,
    interpolated by Triangle::getSurface on the device.  The oracle gets the same corner normals."""
    sc = scenes.cornell_soup(40, seed=5, res=(48, 40))
    n_lat, n_lon, radius, centre = 8, 12, 0.5, np.array([0.0, 0.1, -0.35], np.float32)
    pts = [centre + radius * np.array([0, 0, 1], np.float32)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            pts.append(centre + radius * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], np.float32))
    pts.append(centre - radius * np.array([0, 0, 1], np.float32))
    pts = np.array(pts, np.float32)
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    tris = []
    for j in range(n_lon):
        tris.append((0, ring(1, j), ring(1, j + 1)))
        tris.append((len(pts) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
        for i in range(1, n_lat - 1):
            tris += [(ring(i, j), ring(i + 1, j), ring(i, j + 1)), (ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1))]
    tris = np.array(tris, np.int32)
    # one shared-vertex mesh: the sphere through addVertex / addTriangle so that smoothMesh sees the sharing
    yi = Interface()
    yi.startScene(0)
    handles = []
    for i, m in enumerate(sc["materials"]):
        yi.paramsClearAll(); yi.paramsSet({k: (("color",) + tuple(float(x) for x in v) + (1.0,) if k in ("color", "mirror_color", "diffuse_color") else v) for k, v in m.items()})
        handles.append(yi.createMaterial(f"mat{i}"))
    for i, l in enumerate(sc["lights"]):
        yi.paramsClearAll(); yi.paramsSet({k: (("color",) + tuple(float(x) for x in v) + (1.0,) if k == "color" else v) for k, v in l.items()})
        yi.createLight(f"light{i}")
    yi.paramsClearAll(); yi.paramsSet(dict(sc["camera"], type="perspective")); yi.createCamera("cam")
    yi.paramsClearAll(); yi.paramsSet({"type": "pathtracing", "path_samples": 1, "bounces": 2, "russian_roulette_min_bounces": 2, "caustic_type": "none"}); yi.createIntegrator("default")
    yi.paramsClearAll(); yi.paramsSet({"type": "none"}); yi.createIntegrator("volintegr")
    yi.startGeometry()
    walls = np.asarray(sc["verts"], np.float32).reshape(-1, 3, 3)
    wid = yi.getNextFreeId()
    yi.startTriMesh(wid, 3 * len(walls), len(walls), False, False, 0)
    for t in range(len(walls)):
        yi.addTriangles(walls[t], np.arange(3, dtype=np.int32), handles[int(sc["tri_mat"][t])])
    yi.endTriMesh()
    sid = yi.getNextFreeId()
    yi.startTriMesh(sid, len(pts), len(tris), False, False, 0)
    for p in pts:
        yi.addVertex(float(p[0]), float(p[1]), float(p[2]))
    for t in tris:
        yi.addTriangle(int(t[0]), int(t[1]), int(t[2]), handles[0])
    yi.endTriMesh()
    assert yi.smoothMesh(sid, angle)
    corner = yi.getMeshCornerNormals(sid, len(tris))
    yi.endGeometry()
    rd = scenes.render_settings(48, 40, 6, bounces=2)
    yi.paramsClearAll()
    yi.paramsSet({"camera_name": "cam", "integrator_name": "default", "volintegrator_name": "volintegr", "width": 48, "height": 40,
                  "AA_passes": 1, "AA_minsamples": 6, "AA_pixelwidth": 1.0, "filter_type": "box", "tile_size": 32})
    yi.render()
    film, st = yi.getFilm(48, 40), yi.getRenderStats()
    osc_scene = dict(sc)
    osc_scene["verts"] = np.concatenate([walls, pts[tris]], axis=0)
    osc_scene["tri_mat"] = np.concatenate([np.asarray(sc["tri_mat"], np.int32), np.zeros(len(tris), np.int32)])
    osc_scene["vnormals"] = np.concatenate([np.zeros_like(walls), corner], axis=0)
    ofilm, ost = po.OracleScene(osc_scene).render(rd)
    assert st.n_triangles == len(walls) + len(tris)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"smoothMesh {angle}")
    flat = dict(osc_scene); flat["vnormals"] = None
    ffilm, _ = po.OracleScene(flat).render(rd)
    assert not np.allclose(po.film_to_rgb(ffilm), po.film_to_rgb(ofilm), rtol=1e-3), "smoothing changes the shading"


def test_chunked_frames(monkeypatch):
    """A frame larger than one wavefront chunk (YAFGPU_WF_CHUNK caps the paths in flight): pixel tables, masks of the
    adaptive passes, lens streams and film accumulation must not depend on where the chunk borders fall."""
    sc = scenes.cornell_soup(500, seed=17, res=(100, 90))
    sc["camera"] = dict(sc["camera"], aperture=0.05, dof_distance=3.9, bokeh_type="pentagon")
    rd = scenes.render_settings(100, 90, 12, bounces=2, AA_passes=3, AA_inc_samples=9, AA_threshold=0.03, background=(0.1, 0.2, 0.3))
    def render():
        yi = Interface()
        scenes.load_scene(yi, sc, rd)
        yi.render()
        return yi.getFilm(100, 90), yi.getRenderStats()
    whole, st_w = render()
    monkeypatch.setenv("YAFGPU_WF_CHUNK", "65536")          # 100*90*12 = 108000 paths: two chunks in pass 0
    parts, st_p = render()
    assert st_w.camera_samples == st_p.camera_samples and st_w.rays_closest == st_p.rays_closest and st_w.rays_shadow == st_p.rays_shadow
    assert np.array_equal(whole, parts), "chunked render differs from the one-chunk render"
    assert len(np.unique(np.round(whole[..., 4]))) >= 2      # the adaptive passes did resample a subset


def test_transparent_shadows_flag_with_opaque_materials():
    """transpShad = true selects TriKdTree::intersectTs (kdtree_triangle.cc:983-1162).  Even with no transparent
    material it is not intersectS: it accepts hits from the shadow ray's tmin_ on (:1099), intersectS from 0 on (:936),
    both measured from the origin Scene::isShadowed has already advanced by tmin_ — so an occluder within the bias
    of the surface shadows it under one and not under the other.  The tilted soup puts triangles that close."""
    sc = scenes.cornell_soup(400, seed=4, res=(40, 32), sigma=0.1)
    films = {}
    for transp in (True, False):
        rd = scenes.render_settings(40, 32, 6, bounces=2, path_samples=2, transpShad=transp, adv_auto_shadow_bias_enabled=False, adv_shadow_bias_value=0.02)
        film, st, ofilm, ost = render_both(sc, rd)
        assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
        compare_films(film, ofilm, f"opaque scene, transpShad {transp}")
        films[transp] = film
    assert not np.array_equal(films[True], films[False]), "the scene has occluders inside the bias: the two differ"


@pytest.mark.parametrize("raydepth,integrator", [(1, "pathtracing"), (3, "pathtracing"), (5, "pathtracing"), (4, "directlighting")])
def test_recursive_raytrace_mirror_and_transparency(raydepth, integrator):
    """recursiveRaytrace's perfect specular branch (integrator_montecarlo.cc:971-1025) for shinydiffusemat's mirror
    (with and without Fresnel) and transparency (filtered, straight through): a full integrate() per followed ray, one
    level deeper, alpha from the transmitted ray.  Frames per level behind the parked records; the iteration loop
    runs until the queues are empty."""
    sc = scenes.cornell_soup(260, seed=13, res=(48, 40))
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"][0].update({"specular_reflect": 0.5, "mirror_color": (0.9, 0.9, 1.0)})
    sc["materials"][1].update({"transparency": 0.5, "transmit_filter": 0.6, "specular_reflect": 0.3, "fresnel_effect": True, "IOR": 1.4})
    sc["materials"][2].update({"transparency": 0.7, "transmit_filter": 0.2})
    rd = scenes.render_settings(48, 40, 4, bounces=2, integrator=integrator, raydepth=raydepth, background=(0.2, 0.3, 0.4),
                                bg_transp=True, bg_transp_refract=True)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"recursive raytrace depth {raydepth} {integrator}")
    flat, _ = po.OracleScene(sc).render(dict(rd, raydepth=0))
    assert not np.allclose(po.film_to_rgb(flat), po.film_to_rgb(ofilm), rtol=1e-3), "the recursion changes the image"


@pytest.mark.parametrize("raydepth", [2, 6])
def test_glass_and_mirror_materials(raydepth):
    """GlassMaterial (refraction, Fresnel reflection, total inner reflection, the level-3 cut of reflections inside the
    glass, with and without fake shadows) and MirrorMaterial through recursiveRaytrace and as path bounces."""
    sc = scenes.cornell_soup(300, seed=29, res=(52, 44), sigma=0.06)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.7, 0.95, 0.8), "transmit_filter": 0.9, "mirror_color": (1.0, 0.95, 0.9)})
    sc["materials"].append({"type": "mirror", "color": (0.9, 0.85, 0.7), "reflect": 0.9})
    sc["materials"].append({"type": "glass", "IOR": 1.9, "filter_color": (1.0, 0.6, 0.6), "transmit_filter": 0.5, "fake_shadows": True})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    free = np.arange(10, len(tm))                     # the soup triangles (the first ten are the walls)
    tm[free[0::3]] = nm - 3; tm[free[1::5]] = nm - 2; tm[free[2::7]] = nm - 1
    sc["tri_mat"] = tm
    rd = scenes.render_settings(52, 44, 4, bounces=3, raydepth=raydepth, background=(0.3, 0.3, 0.5), bg_transp=True, bg_transp_refract=True)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"glass + mirror, raydepth {raydepth}")


@pytest.mark.parametrize("raydepth,bounces", [(4, 3), (7, 4)])
def test_glass_absorption(raydepth, bounces):
    """Glass with "absorption": the material owns a BeerVolumeHandler (material_glass.cc:371-398); light that travelled
    inside it is attenuated by exp(-sigma * distance) — for followed specular rays in recursiveRaytrace
    (integrator_montecarlo.cc:991-994, 1016-1019; a ray that leaves the scene from inside comes back black) and for
    path segments that end on the inner side of the surface (integrator_path_tracer.cc:276-279)."""
    sc = scenes.cornell_soup(240, seed=37, res=(52, 44), sigma=0.12)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "glass", "IOR": 1.45, "filter_color": (0.95, 0.95, 1.0), "transmit_filter": 0.6,
                            "absorption": (0.3, 0.8, 0.95), "absorption_dist": 0.35})
    sc["materials"].append({"type": "glass", "IOR": 1.7, "absorption": (0.9, 0.2, 0.0)})          # default distance 1; a zero channel
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    free = np.arange(10, len(tm))
    tm[free[0::2]] = nm - 2; tm[free[1::4]] = nm - 1
    sc["tri_mat"] = tm
    rd = scenes.render_settings(52, 44, 4, bounces=bounces, raydepth=raydepth, background=(0.3, 0.3, 0.5))
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"glass absorption, raydepth {raydepth}")
    clear = dict(sc); clear["materials"] = [{k: v for k, v in m.items() if not k.startswith("absorption")} for m in sc["materials"]]
    cfilm, _ = po.OracleScene(clear).render(rd)
    assert po.film_to_rgb(cfilm)[..., :3].sum() > po.film_to_rgb(ofilm)[..., :3].sum() * 1.02, "absorption darkens the image"


@pytest.mark.parametrize("shadow_depth", [1, 5])
def test_transparent_shadows(shadow_depth):
    """Shadow rays through transparent shinydiffuse and fake-shadow glass are filtered, not blocked
    (TriKdTree::intersectTs; integrator_montecarlo.cc:102-114,176-182,304-309); more than shadowDepth transparent
    surfaces block.  The product of the filters is taken in visiting order, which is the tree's: tolerance, not bits."""
    sc = scenes.cornell_soup(420, seed=31, res=(48, 40), sigma=0.09)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "shinydiffusemat", "color": (0.3, 0.9, 0.4), "diffuse_reflect": 0.6, "transparency": 0.7, "transmit_filter": 0.8,
                            "specular_reflect": 0.2, "fresnel_effect": True, "IOR": 1.3})
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.9, 0.5, 0.5), "transmit_filter": 0.7, "fake_shadows": True})
    tm = np.array(sc["tri_mat"], np.int32)
    free = np.arange(10, len(tm))
    nm = len(sc["materials"])
    tm[free[0::2]] = nm - 2; tm[free[1::4]] = nm - 1
    sc["tri_mat"] = tm
    rd = scenes.render_settings(48, 40, 4, bounces=2, raydepth=2, transpShad=True, shadowDepth=shadow_depth)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"transparent shadows, depth {shadow_depth}", exact_weights=True)
    opaque, _ = po.OracleScene(sc).render(dict(rd, transpShad=False))
    assert po.film_to_rgb(ofilm)[..., :3].sum() > po.film_to_rgb(opaque)[..., :3].sum() * 1.02, "filtered shadows let light through"


def test_coated_glossy_material():
    """CoatedGlossyMaterial (as_diffuse): Blinn lobe + diffuse substrate under a Fresnel-weighted specular coat that
    recursiveRaytrace follows (material_coated_glossy.cc)."""
    sc = scenes.cornell_soup(300, seed=37, res=(48, 40), sigma=0.07)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "coated_glossy", "color": (0.9, 0.8, 0.7), "diffuse_color": (0.3, 0.5, 0.7), "mirror_color": (1.0, 0.95, 0.9),
                            "diffuse_reflect": 0.5, "glossy_reflect": 0.6, "exponent": 80.0, "specular_reflect": 0.8, "IOR": 1.6})
    sc["materials"].append({"type": "coated_glossy", "color": (1.0, 1.0, 1.0), "glossy_reflect": 0.9, "exponent": 300.0, "IOR": 1.0})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[0:4] = nm - 2                                   # two walls
    free = np.arange(10, len(tm)); tm[free[0::3]] = nm - 1
    sc["tri_mat"] = tm
    rd = scenes.render_settings(48, 40, 6, bounces=3, raydepth=3)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "coated glossy")


def test_anisotropic_glossy_lobe():
    """The Ashikhmin-Shirley lobe of glossy / coated_glossy (`anisotropic`, exp_u / exp_v; material_utils_microfacet.h:38-87) in a
    path-traced box: MIS pairs, bounces and the coat's recursion all sample it.  Its sampling calls libm's tanf (double tan
    narrowed on the device): the tolerance is north_star's, the ray counts must still agree."""
    sc = scenes.cornell_soup(300, seed=41, res=(48, 40), sigma=0.07)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "glossy", "color": (0.9, 0.8, 0.85), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.5, "glossy_reflect": 0.5,
                            "anisotropic": True, "exp_u": 400.0, "exp_v": 12.0})
    sc["materials"].append({"type": "glossy", "color": (1.0, 1.0, 1.0), "glossy_reflect": 0.9, "anisotropic": True, "exp_u": 8.0, "exp_v": 900.0})
    sc["materials"].append({"type": "coated_glossy", "color": (0.9, 0.9, 0.8), "diffuse_color": (0.2, 0.6, 0.5), "diffuse_reflect": 0.6, "glossy_reflect": 0.5,
                            "specular_reflect": 0.7, "IOR": 1.5, "anisotropic": True, "exp_u": 30.0, "exp_v": 250.0})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[0:2] = nm - 3; tm[4:6] = nm - 2                 # floor, back wall
    free = np.arange(10, len(tm)); tm[free[0::3]] = nm - 1; tm[free[1::5]] = nm - 3
    sc["tri_mat"] = tm
    rd = scenes.render_settings(48, 40, 6, bounces=3, raydepth=2)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "anisotropic glossy")


@pytest.mark.parametrize("raydepth,integrator", [(1, "pathtracing"), (2, "pathtracing"), (3, "pathtracing"), (2, "directlighting")])
def test_glossy_branch_of_recursive_raytrace(raydepth, integrator):
    """recursiveRaytrace's glossy branch (integrator_montecarlo.cc:861-972): glossy / coated_glossy with as_diffuse off are not
    path-traced but followed by 8 trajectories through the glossy lobe, each a full integrate() one level down with the
    trajectory-splitting state set — fewer light samples (:154) and path samples (:182), shifted first-segment samples (:201-205),
    one trajectory per level below the first (:869).  Mirrors and glass in the scene nest the specular branch inside it and the
    other way round."""
    sc = scenes.cornell_soup(260, seed=43, res=(40, 32), sigma=0.08)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["lights"] = [dict(l, samples=4) for l in sc["lights"]]
    sc["materials"].append({"type": "glossy", "color": (0.9, 0.8, 0.85), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.5, "glossy_reflect": 0.5,
                            "exponent": 60.0, "as_diffuse": False})
    sc["materials"].append({"type": "glossy", "color": (1.0, 0.9, 0.8), "glossy_reflect": 0.9, "as_diffuse": False, "anisotropic": True, "exp_u": 20.0, "exp_v": 300.0})
    sc["materials"].append({"type": "coated_glossy", "color": (0.9, 0.9, 0.8), "diffuse_color": (0.2, 0.6, 0.5), "diffuse_reflect": 0.4, "glossy_reflect": 0.6,
                            "exponent": 150.0, "specular_reflect": 0.7, "IOR": 1.5, "as_diffuse": False})
    sc["materials"].append({"type": "mirror", "color": (0.9, 0.9, 0.9), "reflect": 0.9})
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.8, 0.9, 1.0), "transmit_filter": 0.6})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[0:2] = nm - 5; tm[4:6] = nm - 3; tm[6:8] = nm - 2          # floor glossy, back wall coated, left wall mirror
    free = np.arange(10, len(tm)); tm[free[0::4]] = nm - 4; tm[free[1::6]] = nm - 1; tm[free[2::7]] = nm - 5
    sc["tri_mat"] = tm
    rd = scenes.render_settings(40, 32, 3, bounces=2, raydepth=raydepth, path_samples=8, integrator=integrator)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"glossy branch raydepth {raydepth} {integrator}")


@pytest.mark.parametrize("raydepth,integrator,extra", [(0, "pathtracing", {"no_recursive": True, "bounces": 3}), (1, "pathtracing", {}), (2, "pathtracing", {"bg_transp": True, "bg_transp_refract": True}),
                                                       (3, "pathtracing", {"transpShad": True, "shadowDepth": 3}), (2, "directlighting", {"transpShad": True, "bg_transp_refract": True})])
def test_rough_glass(raydepth, integrator, extra):
    """RoughGlassMaterial (material_rough_glass.cc): a glossy lobe that reflects AND transmits.  recursiveRaytrace's glossy branch takes the
    two-direction sample and sends two rays per trajectory (integrator_montecarlo.cc:919-959: absorption along either, the second one's
    alpha for the level); path segments take the one-direction sample; fake shadows filter the light through getTransparency; glossy,
    mirror and glass in the scene nest the other branches inside it and the other way round."""
    sc = scenes.cornell_soup(260, seed=53, res=(40, 32), sigma=0.08)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["lights"] = [dict(l, samples=2) for l in sc["lights"]]
    sc["materials"].append({"type": "rough_glass", "IOR": 1.5, "alpha": 0.3, "filter_color": (0.8, 0.9, 1.0), "transmit_filter": 0.6, "mirror_color": (1.0, 0.95, 0.9)})
    sc["materials"].append({"type": "rough_glass", "IOR": 1.33, "alpha": 0.8, "filter_color": (0.9, 0.7, 0.8), "transmit_filter": 0.9, "fake_shadows": True,
                            "absorption": (0.4, 0.7, 0.9), "absorption_dist": 0.5, "additionaldepth": 1})
    sc["materials"].append({"type": "rough_glass", "IOR": 2.1, "alpha": 0.05, "fake_shadows": True, "visibility": "no_shadows"})
    sc["materials"].append({"type": "glossy", "color": (0.9, 0.8, 0.85), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.5, "glossy_reflect": 0.5,
                            "exponent": 60.0, "as_diffuse": False})
    sc["materials"].append({"type": "mirror", "color": (0.9, 0.9, 0.9), "reflect": 0.9})
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.8, 0.9, 1.0), "transmit_filter": 0.6})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[4:6] = nm - 6; tm[6:8] = nm - 2          # back wall rough glass (the background shows through it), left wall mirror
    free = np.arange(10, len(tm)); tm[free[0::4]] = nm - 6; tm[free[1::5]] = nm - 5; tm[free[2::7]] = nm - 4; tm[free[3::9]] = nm - 3; tm[free[5::11]] = nm - 1
    sc["tri_mat"] = tm
    rd = scenes.render_settings(40, 32, 3, **dict(dict(bounces=2, raydepth=raydepth, path_samples=4, integrator=integrator, background=(0.2, 0.3, 0.5)), **extra))
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"rough glass raydepth {raydepth} {integrator} {extra}")


@pytest.mark.parametrize("integrator,samples", [("pathtracing", (5, 2)), ("pathtracing", (1, 1)), ("directlighting", (4, 3))])
def test_two_shadow_pairs_per_park(integrator, samples):
    """WfArgs::multi: a vertex whose light estimate has another MIS pair to go — the light's next sample, the next light — parks for two pairs
    at once (odd counts leave a single one at the end; the last pair of an estimate still takes the next segment beside it).  The shadow answers
    steer nothing, so the film must be the one-pair-per-park program's bit for bit, and the oracle's."""
    import os
    sc = scenes.cornell_soup(300, seed=61, res=(48, 40), sigma=0.08, n_lights=2)
    sc["lights"] = [dict(l, samples=n) for l, n in zip(sc["lights"], samples)] + [{"type": "pointlight", "from": (0.3, -0.2, 0.5), "color": (1.0, 0.9, 0.8), "power": 1.5}]
    rd = scenes.render_settings(48, 40, 3, bounces=3, raydepth=0, path_samples=2, integrator=integrator)
    film, st, ofilm, ost = _render_with_rand_state(sc, rd, same_tree=True)
    assert (st.rays_closest, st.rays_shadow) == (ost.rays_closest, ost.rays_shadow)
    compare_films(film, ofilm, f"two pairs per park {integrator} {samples}")
    os.environ["YAFGPU_MULTI_PAIR"] = "0"
    try:
        film1, st1, _, _ = _render_with_rand_state(sc, rd, same_tree=True)
    finally:
        os.environ.pop("YAFGPU_MULTI_PAIR", None)
    assert (st1.rays_closest, st1.rays_shadow) == (st.rays_closest, st.rays_shadow)
    assert np.array_equal(film.view(np.uint32), film1.view(np.uint32)), "one pair per park gives another film"


@pytest.mark.parametrize("raydepth,extra", [(0, {}), (2, {"russian_roulette_min_bounces": 1}), (1, {"no_recursive": True, "path_samples": 2})])
def test_path_caustics(raydepth, extra):
    """caustic_type "path" — PathIntegrator's default when the parameter is absent (integrator_path_tracer.cc:36, :85): after a bounce through a
    specular, glossy or filter lobe the next vertex shows its lights (the emitting panel of the ceiling, a light material) and adds its emission
    after the roulette test (:252-253, :290); the state is left as the last bounce set it for whatever recursiveRaytrace does next (:863, :973)."""
    sc = scenes.cornell_soup(260, seed=59, res=(40, 32), sigma=0.08)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "mirror", "color": (0.9, 0.9, 0.9), "reflect": 0.9})
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.8, 0.9, 1.0), "transmit_filter": 0.6, "fake_shadows": True})
    sc["materials"].append({"type": "glossy", "color": (0.9, 0.8, 0.85), "diffuse_color": (0.5, 0.4, 0.6), "diffuse_reflect": 0.5, "glossy_reflect": 0.5,
                            "exponent": 60.0, "as_diffuse": False})
    sc["materials"].append({"type": "shinydiffusemat", "color": (0.9, 0.6, 0.3), "diffuse_reflect": 0.6, "specular_reflect": 0.5, "emit": 0.8})
    sc["materials"].append({"type": "rough_glass", "IOR": 1.4, "alpha": 0.4, "filter_color": (0.9, 0.9, 0.7), "transmit_filter": 0.5})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[6:8] = nm - 5          # left wall mirror
    free = np.arange(10, len(tm)); tm[free[0::4]] = nm - 4; tm[free[1::5]] = nm - 3; tm[free[2::6]] = nm - 2; tm[free[3::7]] = nm - 1
    sc["tri_mat"] = tm
    kw = dict(bounces=4, raydepth=raydepth, path_samples=3, integrator="pathtracing", caustic_type="path")
    kw.update(extra)
    rd = scenes.render_settings(40, 32, 3, **kw)
    # (with roulette on the tiles' streams are serial state: both sides start from the same libc rand() state)
    both = (lambda s_, r_: _render_with_rand_state(s_, r_, same_tree=True)) if "russian_roulette_min_bounces" in extra else render_both
    film, st, ofilm, ost = both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"path caustics raydepth {raydepth} {extra}")
    film0, _, ofilm0, _ = both(sc, dict(rd, caustic_type="none"))
    assert not np.allclose(ofilm, ofilm0, rtol=1e-3, atol=1e-4), "the scene does not exercise the caustic terms"


@pytest.mark.parametrize("raydepth", [0, 1, 2])
def test_additional_depth_and_transparent_bias(raydepth):
    """Material::additional_depth_ (integrate() carries the largest one met on the way down and recursiveRaytrace goes that much
    deeper below it, integrator_path_tracer.cc:149, integrator_montecarlo.cc:791) on glass, shinydiffuse and glossy, and
    shinydiffusemat's transparent bias (the transmitted ray starts `factor` [x raylevel] along its direction, :1003-1011)."""
    sc = scenes.cornell_soup(260, seed=47, res=(40, 32), sigma=0.08)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.8, 0.9, 1.0), "transmit_filter": 0.6, "additionaldepth": 2})
    sc["materials"].append({"type": "shinydiffusemat", "color": (0.5, 0.7, 0.9), "diffuse_reflect": 0.6, "transparency": 0.7, "transmit_filter": 0.8,
                            "additionaldepth": 1, "transparentbias_factor": 0.01, "transparentbias_multiply_raydepth": True})
    sc["materials"].append({"type": "shinydiffusemat", "color": (0.9, 0.7, 0.5), "diffuse_reflect": 0.7, "transparency": 0.5, "specular_reflect": 0.3,
                            "transparentbias_factor": 0.02})
    sc["materials"].append({"type": "glossy", "color": (0.9, 0.9, 0.9), "glossy_reflect": 0.8, "exponent": 100.0, "as_diffuse": False, "additionaldepth": 1})
    tm = np.array(sc["tri_mat"], np.int32)
    nm = len(sc["materials"])
    tm[4:6] = nm - 1                                                   # back wall glossy
    free = np.arange(10, len(tm)); tm[free[0::4]] = nm - 4; tm[free[1::4]] = nm - 3; tm[free[2::5]] = nm - 2
    sc["tri_mat"] = tm
    rd = scenes.render_settings(40, 32, 3, bounces=2, raydepth=raydepth, path_samples=2)
    film, st, ofilm, ost = render_both(sc, rd)
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, f"additional depth / transparent bias, raydepth {raydepth}")
    yi = Interface(strict=False)
    scenes.load_scene(yi, sc, dict(rd, raydepth=6))
    assert not yi.render() and "7" in yi.getLastError(), yi.getLastError()          # 6 + 2 frames


def test_light_count_and_sample_count_limits():
    """The light-estimate bookkeeping packs the light index in 8 bits and the sample index in 12: 255 lights render and equal
    the oracle, 256 are refused; an area light asking for more than 4095 samples per estimate is refused."""
    sc = scenes.cornell_soup(120, seed=51, res=(24, 20), sigma=0.1)
    rng = np.random.default_rng(7)
    points = [{"type": "pointlight", "from": tuple(float(x) for x in rng.uniform(-0.8, 0.8, 3)), "color": (1.0, 0.9, 0.8), "power": 0.02} for _ in range(255)]
    rd = scenes.render_settings(24, 20, 1, integrator="directlighting")
    sc255 = dict(sc, lights=list(sc["lights"]) + points[:254])
    yi = Interface()
    scenes.load_scene(yi, sc255, rd)
    yi.render()
    film, st = yi.getFilm(24, 20), yi.getRenderStats()
    # at this resolution three camera rays run exactly into an edge two walls of different colour share: an exact tie in t
    # that TriKdTree::intersect resolves by visiting order, i.e. by tree topology (see test_multi_pass_anti_aliasing) —
    # the oracle walks the product's tree
    from libyafaray_amd import interface
    osc = po.OracleScene(sc255)
    osc.set_tree(*interface.build_kdtree(sc255["verts"], threads=4, device=DEVICE_TREE)[:3])
    ofilm, ost = osc.render(rd)
    assert st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "255 lights")
    yi = Interface(strict=False)
    scenes.load_scene(yi, dict(sc, lights=list(sc["lights"]) + points), rd)
    assert not yi.render() and "255" in yi.getLastError(), yi.getLastError()
    yi = Interface(strict=False)
    scenes.load_scene(yi, dict(sc, lights=[dict(sc["lights"][0], samples=5000)]), rd)
    assert not yi.render() and "4095" in yi.getLastError(), yi.getLastError()


def test_xml_scene_with_every_feature(tmp_path):
    """The C++ XML loader driven with everything the device path does — glass, mirror, coated glossy, mirror /
    transparent shinydiffuse, depth of field, recursion depth, transparent shadows, adaptive multi-pass AA with a
    gauss filter and a sample clamp — against the oracle fed by an independent Python parse of the same file."""
    from tests import xml_scene, xml_writer
    sc = scenes.cornell_soup(240, seed=43, res=(44, 36), sigma=0.08)
    sc["materials"] = [dict(m, type=m.get("type", "shinydiffusemat")) for m in sc["materials"]]
    sc["materials"][0].update({"specular_reflect": 0.3, "mirror_color": (0.9, 0.9, 1.0)})
    sc["materials"] += [
        {"type": "glass", "IOR": 1.5, "filter_color": (0.8, 0.95, 0.85), "transmit_filter": 0.9, "fake_shadows": True},
        {"type": "mirror", "color": (0.9, 0.85, 0.7), "reflect": 0.9},
        {"type": "coated_glossy", "color": (0.9, 0.8, 0.7), "diffuse_color": (0.3, 0.5, 0.7), "diffuse_reflect": 0.5, "glossy_reflect": 0.6,
         "exponent": 80.0, "specular_reflect": 0.8, "IOR": 1.6},
        {"type": "shinydiffusemat", "color": (0.4, 0.8, 0.5), "diffuse_reflect": 0.6, "transparency": 0.6, "transmit_filter": 0.7},
    ]
    tm = np.array(sc["tri_mat"], np.int32)
    free = np.arange(10, len(tm)); nm = len(sc["materials"])
    for k in range(4):
        tm[free[k::6]] = nm - 4 + k
    sc["tri_mat"] = tm
    sc["camera"] = dict(sc["camera"], aperture=0.03, dof_distance=3.8, bokeh_type="hexagon", bokeh_rotation=15.0)
    rd = scenes.render_settings(44, 36, 3, bounces=2, raydepth=3, transpShad=True, shadowDepth=3, background=(0.2, 0.25, 0.4),
                                AA_passes=3, AA_inc_samples=2, AA_threshold=0.02, AA_clamp_samples=2.0, filter_type="gauss", AA_pixelwidth=1.5)
    path = str(tmp_path / "everything.xml")
    xml_writer.write(path, sc, rd)
    yi = Interface()
    yi.loadXml(path)
    yi.render()
    film, st = yi.getFilm(44, 36), yi.getRenderStats()
    osc_scene, ord_ = xml_scene.load(path)
    from libyafaray_amd import interface
    osc = po.OracleScene(osc_scene)
    osc.set_tree(*interface.build_kdtree(osc_scene["verts"], threads=4, device=DEVICE_TREE)[:3])      # riVdC(1) == riS(1): see test_multi_pass_anti_aliasing
    ofilm, ost = osc.render(ord_)
    assert st.camera_samples == ost.camera_samples
    assert st.rays_closest == ost.rays_closest and st.rays_shadow == ost.rays_shadow
    compare_films(film, ofilm, "xml scene with every feature", exact_weights=False)


def assert_matches_an_oracle_render(sc, rd, film, st, what):
    # Two oracle renders: the reference's traversal over the PRODUCT's tree (exact hit-distance ties — a camera ray into
    # the shared edge of two wall triangles — resolve by the order leaves are visited in) and over the oracle's own
    # reference-style tree (the reference's walk skips a leaf the ray enters exactly where it leaves the node above — a
    # ray into the corner edge of two walls that are both split planes — which its own builder's layout does not expose
    # but a foreign tree can).  The device must agree with one of them on every pixel and as a whole on the counts.
    osc = po.OracleScene(sc)
    own_film, own_st = osc.render(rd)
    osc.set_tree(*interface.build_kdtree(sc["verts"], threads=4, device=DEVICE_TREE)[:3])
    ofilm, ost = osc.render(rd)
    assert st.camera_samples in (ost.camera_samples, own_st.camera_samples), "resampled sets differ"
    def close(f, o):
        a, b = po.film_to_rgb(f), po.film_to_rgb(o)
        rel = np.abs(a[..., :3] - b[..., :3]) / np.maximum(np.abs(b[..., :3]), ABS_FLOOR)
        return (rel.max(axis=-1) <= RTOL) & np.isclose(a[..., 3], b[..., 3], rtol=1e-5, atol=1e-6) & np.isclose(f[..., 4], o[..., 4], rtol=2e-6)
    ok_prod, ok_own = close(film, ofilm), close(film, own_film)
    print(f"{what}: pixels matching product-tree oracle {ok_prod.mean():.4f}, own-tree oracle {ok_own.mean():.4f}")
    neither = int((~(ok_prod | ok_own)).sum())
    # a wide filter spreads each of the two artefacts over its neighbours: a pixel that receives both matches neither
    wide = rd.get("filter_type", "box") != "box" or rd.get("AA_pixelwidth", 1.0) > 1.002
    assert neither == 0 or (wide and neither <= 4 and not ok_prod.all() and not ok_own.all()), f"{what}: {neither} pixels match neither oracle render"
    assert ok_prod.mean() > 0.95 or ok_own.mean() > 0.95      # mirror rooms send many rays into wall corners: both artefacts at once
    rays = (st.rays_closest, st.rays_shadow)
    if ok_prod.all():
        assert rays == (ost.rays_closest, ost.rays_shadow)
    elif ok_own.all():
        assert rays == (own_st.rays_closest, own_st.rays_shadow)


def _random_material(rng):
    kind = rng.choice(["sd", "sd_mirror", "sd_transp", "sd_transl", "glossy", "coated", "glass", "glass_abs", "mirror"])
    col = lambda lo=0.2, hi=1.0: tuple(float(x) for x in rng.uniform(lo, hi, 3))
    if kind == "sd":
        m = {"type": "shinydiffusemat", "color": col(), "diffuse_reflect": float(rng.uniform(0.4, 1.0)), "emit": float(rng.choice([0.0, 0.0, 0.3]))}
        if rng.random() < 0.3:
            m.update({"diffuse_brdf": "oren_nayar", "sigma": float(rng.uniform(0.05, 0.5))})
        return m
    if kind == "sd_mirror":
        return {"type": "shinydiffusemat", "color": col(), "diffuse_reflect": 0.7, "specular_reflect": float(rng.uniform(0.2, 0.8)), "mirror_color": col(0.7),
                "fresnel_effect": bool(rng.random() < 0.5), "IOR": float(rng.uniform(1.2, 2.0))}
    if kind == "sd_transp":
        return {"type": "shinydiffusemat", "color": col(), "diffuse_reflect": 0.6, "transparency": float(rng.uniform(0.3, 0.9)), "transmit_filter": float(rng.uniform(0.0, 1.0))}
    if kind == "sd_transl":
        return {"type": "shinydiffusemat", "color": col(), "diffuse_reflect": 0.6, "translucency": float(rng.uniform(0.2, 0.6)), "transmit_filter": float(rng.uniform(0.0, 1.0))}
    if kind == "glossy":
        return {"type": "glossy", "color": col(0.6), "diffuse_color": col(), "diffuse_reflect": float(rng.uniform(0.0, 0.6)), "glossy_reflect": float(rng.uniform(0.3, 0.9)),
                "exponent": float(rng.uniform(5, 400)), "as_diffuse": bool(rng.random() < 0.6),
                **({"anisotropic": True, "exp_u": float(rng.uniform(2, 600)), "exp_v": float(rng.uniform(2, 600))} if rng.random() < 0.3 else {})}
    if kind == "coated":
        return {"type": "coated_glossy", "color": col(0.6), "diffuse_color": col(), "mirror_color": col(0.8), "diffuse_reflect": float(rng.uniform(0.0, 0.6)),
                "glossy_reflect": float(rng.uniform(0.3, 0.9)), "exponent": float(rng.uniform(5, 400)), "specular_reflect": float(rng.uniform(0.3, 1.0)),
                "IOR": float(rng.uniform(1.1, 2.2)), "as_diffuse": bool(rng.random() < 0.6)}
    if kind in ("glass", "glass_abs"):
        m = {"type": "glass", "IOR": float(rng.uniform(1.1, 2.2)), "filter_color": col(0.5), "transmit_filter": float(rng.uniform(0.0, 1.0)), "mirror_color": col(0.8),
             "fake_shadows": bool(rng.random() < 0.5)}
        if kind == "glass_abs":
            m.update({"absorption": col(0.05), "absorption_dist": float(rng.uniform(0.1, 2.0))})
        return m
    return {"type": "mirror", "color": col(0.6), "reflect": float(rng.uniform(0.5, 1.0))}


def _push_to_extremes(m, rng):
    """Parameter values at the ends of their ranges: lobes that switch off, exponents at the clamp, IOR 1, black colours."""
    ends = {"diffuse_reflect": [0.0, 1.0], "specular_reflect": [0.0, 1.0], "transparency": [0.0, 1.0], "translucency": [0.0, 1.0],
            "transmit_filter": [0.0, 1.0], "glossy_reflect": [0.0, 1.0], "exponent": [1.0, 2.0, 1e4, 1e6], "IOR": [1.0, 1.0001, 3.5],
            "emit": [0.0, 5.0], "reflect": [0.0, 1.0], "sigma": [0.0, 1.0], "absorption_dist": [1e-3, 50.0]}
    for k in list(m):
        if k in ends and rng.random() < 0.5:
            m[k] = float(rng.choice(ends[k]))
        elif k in ("color", "diffuse_color", "mirror_color", "filter_color", "absorption") and rng.random() < 0.3:
            m[k] = tuple(float(x) for x in rng.choice([0.0, 1.0], 3))
    return m


def _feature_mix(seed, textures=True, serial=False):
    """serial: the same mix made to consume the reference's serial state — path tracing with Russian roulette from a random depth on and,
    mostly, a second light (the light counter) — for the exact replay (test_random_feature_mixes_with_serial_state)"""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(36, 60)), int(rng.integers(28, 48))
    # bounce vertices of the path tracer pick ONE light through a counter that is serial state in the reference
    # (SURVEY row N4): several lights only where every light is always estimated
    integrator = str(rng.choice(["pathtracing", "pathtracing", "directlighting"]))
    many_lights = integrator == "directlighting"
    sc = scenes.cornell_soup(int(rng.integers(150, 420)), seed=100 + seed, res=(w, h), sigma=float(rng.uniform(0.05, 0.14)),
                             n_lights=int(rng.integers(1, 3)) if many_lights else 1)
    sc["materials"] = [dict(m) for m in sc["materials"]]
    base = len(sc["materials"])
    sc["materials"] += [_random_material(rng) for _ in range(int(rng.integers(2, 6)))]
    if seed % 4 == 3:
        sc["materials"][base:] = [_push_to_extremes(m, rng) for m in sc["materials"][base:]]
    tm = np.array(sc["tri_mat"], np.int32)
    free = np.arange(10, len(tm))
    pick = rng.random(len(free))
    for k in range(base, len(sc["materials"])):
        lo = (k - base) * 0.15
        tm[free[(pick >= lo) & (pick < lo + 0.15)]] = k
    if rng.random() < 0.5:
        tm[int(rng.integers(0, 5)) * 2: int(rng.integers(0, 5)) * 2 + 2] = int(rng.integers(base, len(sc["materials"])))     # a wall too
    sc["tri_mat"] = tm
    if many_lights and rng.random() < 0.6:
        sc["lights"] = list(sc["lights"]) + [{"type": "pointlight", "from": tuple(float(x) for x in rng.uniform(-0.6, 0.6, 3)),
                                             "color": (1.0, 0.9, 0.8), "power": float(rng.uniform(0.5, 3.0))}]
    if rng.random() < 0.4:
        vn = rng.normal(size=(len(tm), 3, 3)).astype(np.float32) * 0.15
        v = np.asarray(sc["verts"], np.float32).reshape(-1, 3, 3)
        ng = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]); ng /= np.maximum(np.linalg.norm(ng, axis=1, keepdims=True), 1e-20)
        vn = vn + ng[:, None, :]
        vn /= np.linalg.norm(vn, axis=2, keepdims=True)
        vn[:10] = 0.0                                                     # the walls keep their geometric normals
        sc["vnormals"] = vn.reshape(-1, 9).astype(np.float32)
    if rng.random() < 0.4:
        sc["camera"] = dict(sc["camera"], aperture=float(rng.uniform(0.01, 0.08)), dof_distance=float(rng.uniform(3.0, 4.5)),
                            bokeh_type=str(rng.choice(["disk1", "disk2", "triangle", "square", "pentagon", "hexagon", "ring"])),
                            bokeh_bias=str(rng.choice(["uniform", "center", "edge"])), bokeh_rotation=float(rng.uniform(0, 90)))
    kw = dict(bounces=int(rng.integers(1, 5)), raydepth=int(rng.integers(0, 6)), path_samples=int(rng.integers(1, 4)),
              integrator=integrator,
              background=tuple(float(x) for x in rng.uniform(0, 0.5, 3)), bg_transp=bool(rng.random() < 0.3), bg_transp_refract=bool(rng.random() < 0.3),
              transpShad=bool(rng.random() < 0.5), shadowDepth=int(rng.integers(1, 5)), no_recursive=bool(rng.random() < 0.2))
    if rng.random() < 0.35:
        kw.update(AA_passes=int(rng.integers(2, 4)), AA_inc_samples=int(rng.integers(1, 4)), AA_threshold=float(rng.uniform(0.0, 0.05)))
    spp = int(rng.integers(2, 6))
    # second stage: per-material flags, light sampling, film and sampling options
    for m in sc["materials"][base:]:
        if rng.random() < 0.25:
            m["visibility"] = str(rng.choice(["no_shadows", "shadow_only", "invisible"]))
        if rng.random() < 0.2:
            m["receive_shadows"] = False
        if m["type"] == "shinydiffusemat" and rng.random() < 0.2:
            m["flat_material"] = True
    for l in sc["lights"]:
        if l["type"] == "arealight":
            l["samples"] = int(rng.integers(1, 4))
        if rng.random() < 0.2:
            l["cast_shadows"] = False
    if rng.random() < 0.3:
        kw.update(filter_type=str(rng.choice(["box", "gauss", "mitchell", "lanczos"])), AA_pixelwidth=float(rng.uniform(1.0, 3.0)))
    if rng.random() < 0.3:
        kw.update(AA_clamp_samples=float(rng.uniform(0.5, 4.0)))
    if rng.random() < 0.3:
        kw.update(adv_base_sampling_offset=int(rng.integers(0, 5000)), adv_computer_node=int(rng.integers(0, 3)))
    if rng.random() < 0.3:
        kw.update(adv_auto_shadow_bias_enabled=False, adv_shadow_bias_value=float(rng.uniform(1e-4, 2e-2)),
                  adv_auto_min_raydist_enabled=False, adv_min_raydist_value=float(rng.uniform(1e-5, 1e-3)))
    if rng.random() < 0.3:
        kw.update(tile_size=int(rng.choice([8, 16, 32, 64])))
    if rng.random() < 0.3 and "AA_passes" in kw:
        kw.update(AA_detect_color_noise=bool(rng.random() < 0.5), AA_dark_detection_type=str(rng.choice(["none", "linear", "curve"])),
                  AA_dark_threshold_factor=float(rng.uniform(0.0, 1.0)), AA_variance_edge_size=int(rng.integers(4, 12)),
                  AA_variance_pixels=int(rng.integers(0, 3)), AA_resampled_floor=float(rng.uniform(0.0, 20.0)),
                  AA_light_sample_multiplier_factor=float(rng.uniform(1.0, 2.0)), AA_sample_multiplier_factor=float(rng.uniform(1.0, 1.6)))
    if seed % 3 == 2:            # third stage: camera placement and lens, light geometry and strength
        eye = rng.uniform(-0.8, 0.8, 3) if rng.random() < 0.4 else np.array([rng.uniform(-1, 1), -rng.uniform(2.5, 6.0), rng.uniform(-0.8, 0.8)])
        to = rng.uniform(-0.5, 0.5, 3)
        sc["camera"] = dict(sc["camera"], **{"from": tuple(float(x) for x in eye), "to": tuple(float(x) for x in to),
                                             "up": tuple(float(x) for x in (eye + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0]))),
                                             "focal": float(rng.uniform(0.4, 3.0))})
        if rng.random() < 0.5:
            sc["camera"]["aspect_ratio"] = float(rng.uniform(0.6, 1.8))
        for l in sc["lights"]:
            l["power"] = float(l.get("power", 1.0) * 10.0 ** rng.uniform(-1.5, 1.0))
            l["color"] = tuple(float(x) for x in rng.uniform(0.0, 1.0, 3))
            if l["type"] == "arealight" and rng.random() < 0.5:      # a tilted parallelogram instead of the ceiling panel
                c = rng.uniform(-0.6, 0.6, 3); e1 = rng.normal(size=3) * 0.3; e2 = rng.normal(size=3) * 0.3
                l["corner"] = tuple(float(x) for x in c); l["point1"] = tuple(float(x) for x in c + e1); l["point2"] = tuple(float(x) for x in c + e2)
    if rng.random() < 0.25:      # a crop window of the camera's frame
        cw, ch = int(rng.integers(8, w - 4)), int(rng.integers(8, h - 4))
        kw.update(xstart=int(rng.integers(0, w - cw)), ystart=int(rng.integers(0, h - ch)))
        w, h = cw, ch
    rough = seed % 4 == 1
    if rough:      # rough glass on a fifth of the free triangles, from a stream of its own (the draws above stay what they were)
        rr = np.random.default_rng(7000 + seed)
        rcol = lambda lo: tuple(float(x) for x in rr.uniform(lo, 1.0, 3))
        m = {"type": "rough_glass", "IOR": float(rr.uniform(1.1, 2.2)), "alpha": float(rr.choice([rr.uniform(0.02, 1.0), 1e-5, 2.5])), "filter_color": rcol(0.5),
             "transmit_filter": float(rr.uniform(0.0, 1.0)), "mirror_color": rcol(0.8), "fake_shadows": bool(rr.random() < 0.5)}
        if rr.random() < 0.4:
            m.update({"absorption": rcol(0.05), "absorption_dist": float(rr.uniform(0.1, 2.0))})
        if rr.random() < 0.2:
            m["visibility"] = str(rr.choice(["no_shadows", "shadow_only"]))
        sc["materials"].append(m)
        tm = np.array(sc["tri_mat"], np.int32)
        cand = np.arange(10, len(tm))
        tm[cand[rr.random(len(cand)) < 0.2]] = len(sc["materials"]) - 1
        sc["tri_mat"] = tm
        kw["raydepth"] = max(kw["raydepth"], 1)           # (so that the glossy branch of recursiveRaytrace runs at all)
    if serial:
        rs = np.random.default_rng(5000 + seed)
        kw["integrator"] = "pathtracing"
        kw["bounces"] = max(kw["bounces"], 2)
        kw["russian_roulette_min_bounces"] = int(rs.integers(0, kw["bounces"]))
        # (up to 255 integrate() calls per camera sample are replayed: DESIGN.md, serial state; a rough-glass trajectory makes two)
        kw["raydepth"] = min(kw["raydepth"], 2 if rough else 3)
        for m in sc["materials"]:
            m.pop("additionaldepth", None)
        if rs.random() < 0.7:
            sc["lights"] = list(sc["lights"]) + [{"type": "pointlight", "from": tuple(float(x) for x in rs.uniform(-0.6, 0.6, 3)),
                                                 "color": (1.0, 0.9, 0.8), "power": float(rs.uniform(0.5, 3.0))}]
    if seed % 3 == 1:
        kw["caustic_type"] = "path"      # the reference's default when the parameter is absent: path caustics (include_lights_ and emission after a specular / glossy / filter bounce)
    if textures and rng.random() < 0.4:
        _texturize(sc, rng)
    rd = scenes.render_settings(w, h, spp, **kw)
    return sc, rd, w, h, base, kw


def _texturize(sc, rng):
    """image textures and shader-node graphs on the scene's shinydiffuse materials: random textures, texture
    coordinates on every triangle, a random graph on a random subset of the slots the material's lobes make meaningful"""
    n = np.asarray(sc["verts"]).reshape(-1, 3, 3).shape[0]
    sc["uv"] = rng.uniform(-0.5, 2.5, (n, 3, 2)).astype(np.float32)
    if rng.random() < 0.7:
        sc["orco"] = (np.asarray(sc["verts"], np.float32).reshape(-1, 3, 3) * 0.8 + rng.normal(0, 0.05, (n, 3, 3))).astype(np.float32)
    img = lambda: rng.uniform(0, 1, (int(rng.integers(2, 12)), int(rng.integers(2, 12)), 4)).astype(np.float32)
    sc["textures"] = []
    for k in range(int(rng.integers(1, 4))):
        t = dict(name=f"t{k}", texels=img(), interpolate=str(rng.choice(["bilinear", "none"])), clipping=str(rng.choice(["repeat", "extend", "clip", "clipcube", "checker"])),
                 color_space=str(rng.choice(["sRGB", "LinearRGB", "Raw_Manual_Gamma", "XYZ"])), gamma=float(rng.uniform(1.0, 2.4)))
        if rng.random() < 0.4:
            t.update(xrepeat=int(rng.integers(1, 4)), yrepeat=int(rng.integers(1, 4)), mirror_x=bool(rng.random() < 0.5), mirror_y=bool(rng.random() < 0.5))
        if rng.random() < 0.3:
            t.update(rot90=bool(rng.random() < 0.5), cropmin_x=float(rng.uniform(0, 0.3)), cropmax_x=float(rng.uniform(0.6, 1.0)), cropmin_y=float(rng.uniform(0, 0.3)))
        if rng.random() < 0.3:
            t.update(adj_intensity=float(rng.uniform(0.5, 1.5)), adj_contrast=float(rng.uniform(0.5, 1.5)), adj_saturation=float(rng.uniform(0.0, 2.0)),
                     adj_hue=float(rng.uniform(-90, 90)), adj_clamp=bool(rng.random() < 0.5))
        if t["clipping"] == "checker":
            t.update(even_tiles=bool(rng.random() < 0.5), odd_tiles=bool(rng.random() < 0.7), checker_dist=float(rng.uniform(0.0, 0.4)))
        sc["textures"].append(t)
    tex = lambda: str(rng.choice([t["name"] for t in sc["textures"]]))
    texcos = ["uv", "global", "orco", "transformed", "window", "normal"]
    for m in sc["materials"]:
        kind = m.get("type", "shinydiffusemat")
        if kind not in ("shinydiffusemat", "glossy", "coated_glossy", "glass") or rng.random() < 0.4:
            continue
        nodes, k = [], [0]
        def mapper():
            k[0] += 1
            nd = dict(name=f"map{k[0]}", type="texture_mapper", texture=tex(), texco=str(rng.choice(texcos)), mapping=str(rng.choice(["plain", "cube", "tube", "sphere"])),
                      scale=tuple(float(x) for x in rng.uniform(0.5, 3.0, 3)), offset=tuple(float(x) for x in rng.uniform(-0.5, 0.5, 3)))
            if nd["texco"] == "transformed":
                mtx = np.eye(4, dtype=np.float32); mtx[:3, :] = rng.uniform(-1, 1, (3, 4)); nd["transform"] = mtx
            nodes.append(nd)
            return nd["name"]
        def layer(scalar, upper):
            k[0] += 1
            nd = dict(name=f"lay{k[0]}", type="layer", input=mapper(), mode=int(rng.integers(0, 9)), colfac=float(rng.uniform(0.3, 1.0)), valfac=float(rng.uniform(0.3, 1.0)),
                      def_col=tuple(float(x) for x in rng.uniform(0, 1, 3)) + (1.0,), def_val=float(rng.uniform(0, 1)), do_color=not scalar, do_scalar=scalar,
                      color_input=bool(rng.random() < 0.8), noRGB=bool(rng.random() < 0.2), stencil=bool(rng.random() < 0.2), negative=bool(rng.random() < 0.2),
                      use_alpha=bool(rng.random() < 0.2), upper_color=tuple(float(x) for x in rng.uniform(0, 1, 3)) + (1.0,), upper_value=float(upper))
            nodes.append(nd)
            if rng.random() < 0.3:          # a second layer stacked on the first
                k[0] += 1
                top = dict(nd, name=f"lay{k[0]}", input=mapper(), upper_layer=nd["name"], mode=int(rng.integers(0, 9)))
                top.pop("upper_color"); top.pop("upper_value")
                nodes.append(top)
                return top["name"]
            return nd["name"]
        if kind == "glass":
            if rng.random() < 0.6:
                m["filter_color_shader"] = layer(False, 0.0)
            if rng.random() < 0.5:
                m["mirror_color_shader"] = layer(False, 0.0)
            if rng.random() < 0.4:
                m["IOR_shader"] = layer(True, 0.0)
                nodes[-1]["valfac"] = float(rng.uniform(0.1, 0.6))
            if nodes and len(nodes) <= 16:
                m["nodes"] = nodes
            else:
                for key in [key for key in m if key.endswith("_shader")]:
                    m.pop(key)
            continue
        if kind != "shinydiffusemat":      # glossy / coated glossy: their own slots
            if rng.random() < 0.6:
                m["diffuse_shader"] = layer(False, 0.0)
            if rng.random() < 0.6:
                m["glossy_shader"] = layer(False, 0.0)
            if rng.random() < 0.5:
                m["glossy_reflect_shader"] = layer(True, m.get("glossy_reflect", 1.0))
            if rng.random() < 0.4 and not m.get("anisotropic"):
                m["exponent_shader"] = layer(True, m.get("exponent", 50.0))
                nodes[-1]["valfac"] = float(rng.uniform(20.0, 200.0))
            if rng.random() < 0.3:
                m["diffuse_refl_shader"] = layer(True, 1.0)
            if kind == "coated_glossy":
                if rng.random() < 0.5:
                    m["mirror_shader"] = layer(True, m.get("specular_reflect", 1.0))
                if rng.random() < 0.4:
                    m["mirror_color_shader"] = layer(False, 0.0)
                if rng.random() < 0.4:
                    m["IOR_shader"] = layer(True, 0.0)
            if nodes and len(nodes) <= 16:
                m["nodes"] = nodes
            else:
                for key in [key for key in m if key.endswith("_shader")]:
                    m.pop(key)
            continue
        if rng.random() < 0.8:
            if rng.random() < 0.2:
                k[0] += 1
                val = f"val{k[0]}"
                nodes.append(dict(name=val, type="value", color=tuple(float(x) for x in rng.uniform(0, 1, 3)), alpha=1.0, scalar=float(rng.uniform(0, 1))))
                mix = dict(name=f"mix{k[0]}", type="mix", mode=int(rng.integers(0, 10)), input1=mapper(), input2=val, value=float(rng.uniform(0, 1)))
                nodes.append(mix)
                m["diffuse_shader"] = mix["name"]
            else:
                m["diffuse_shader"] = layer(False, 0.0)
        if m.get("specular_reflect", 0.0) > 0 and rng.random() < 0.6:
            m["mirror_shader"] = layer(True, m["specular_reflect"])
            if rng.random() < 0.5:
                m["mirror_color_shader"] = layer(False, 0.0)
            if m.get("fresnel_effect") and rng.random() < 0.5:
                m["IOR_shader"] = layer(True, 0.0)
        if m.get("transparency", 0.0) > 0 and rng.random() < 0.6:
            m["transparency_shader"] = layer(True, m["transparency"])
        if m.get("translucency", 0.0) > 0 and rng.random() < 0.6:
            m["translucency_shader"] = layer(True, m["translucency"])
        if m.get("diffuse_brdf") == "oren_nayar" and rng.random() < 0.6:
            m["sigma_oren_shader"] = layer(True, m.get("sigma", 0.1))
        if rng.random() < 0.3:
            m["diffuse_refl_shader"] = layer(True, m.get("diffuse_reflect", 1.0))
        if nodes and len(nodes) <= 16:
            m["nodes"] = nodes
        else:
            for key in [key for key in m if key.endswith("_shader")]:
                m.pop(key)
    # bump shaders, from a stream of their own (the draws above stay what they were): one layer, sometimes two, over any coordinates
    rb = np.random.default_rng(int(rng.integers(0, 2 ** 31)))
    for t in sc["textures"]:
        if rb.random() < 0.25:
            t["normalmap"] = True      # only a bump shader's mapper reads the flag
    for mi, m in enumerate(sc["materials"]):
        if m.get("type", "shinydiffusemat") not in ("shinydiffusemat", "glossy", "coated_glossy", "glass") or rb.random() < 0.65:
            continue
        nodes = list(m.get("nodes", []))
        if len(nodes) + 4 > 16:
            continue
        def bump_mapper(name):
            nd = dict(name=name, type="texture_mapper", texture=str(rb.choice([t["name"] for t in sc["textures"]])), texco=str(rb.choice(texcos)),
                      mapping=str(rb.choice(["plain", "cube", "tube", "sphere"])), scale=tuple(float(x) for x in rb.uniform(0.5, 3.0, 3)),
                      offset=tuple(float(x) for x in rb.uniform(-0.5, 0.5, 3)), bump_strength=float(rb.uniform(0.2, 4.0)))
            if nd["texco"] == "transformed":
                mtx = np.eye(4, dtype=np.float32); mtx[:3, :] = rb.uniform(-1, 1, (3, 4)); nd["transform"] = mtx
            return nd
        lay = dict(name="bump_a", type="layer", input="bump_map_a", mode=0, valfac=1.0, def_val=1.0, do_color=False, do_scalar=True, color_input=False, upper_value=0.0,
                   negative=bool(rb.random() < 0.3))
        nodes += [lay, bump_mapper("bump_map_a")]
        m["bump_shader"] = "bump_a"
        if rb.random() < 0.3:
            nodes += [dict(lay, name="bump_b", input="bump_map_b", upper_layer="bump_a", negative=bool(rb.random() < 0.3)), bump_mapper("bump_map_b")]
            nodes[-2].pop("upper_value")
            m["bump_shader"] = "bump_b"
        m["nodes"] = nodes


@pytest.mark.parametrize("seed", list(range(int(__import__("os").environ.get("YAFGPU_FUZZ_FIRST", "0")), int(__import__("os").environ.get("YAFGPU_FUZZ_SEEDS", "16")))))
def test_random_feature_mixes(seed, monkeypatch):
    """Features are pinned one at a time above; here random combinations of them — materials of every supported type
    on one scene, area + point lights, vertex normals, depth of field, recursion depth, transparent shadows, path
    samples, background alpha modes, adaptive passes — must still equal the oracle: steps share parked records,
    frames and queues, and a field one feature reuses must not leak into another."""
    sc, rd, w, h, base, kw = _feature_mix(seed)
    if seed % 2:      # every other seed in several wavefront chunks: chunk borders must not show (pixel lists, frames, lens streams)
        monkeypatch.setenv("YAFGPU_WF_CHUNK", str([700, 1500, 4000][seed % 3]))
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film, st = yi.getFilm(w, h), yi.getRenderStats()
    assert_matches_an_oracle_render(sc, rd, film, st, f"feature mix {seed}: {[m['type'] for m in sc['materials'][base:]]} {kw}")


def _random_lights(rng, area):
    """one to four lights of any of the five types, placed in or aimed into the soup's room; `area`: the scene's own ceiling panel"""
    v = lambda lo, hi: tuple(float(x) for x in rng.uniform(lo, hi, 3))
    toward = lambda: (float(rng.uniform(-0.6, 0.6)), float(-rng.uniform(0.3, 1.0)), float(rng.uniform(-0.2, 0.9)))      # out through the open front, or up
    lights = []
    for _ in range(int(rng.integers(1, 5))):
        kind = str(rng.choice(["arealight", "pointlight", "directionallight", "sunlight", "spherelight"]))
        l = {"type": kind, "color": v(0.3, 1.0)}
        if kind == "arealight":
            l = dict(area, samples=int(rng.integers(1, 4)))
            if rng.random() < 0.5:      # a tilted parallelogram instead of the ceiling panel
                c = rng.uniform(-0.6, 0.6, 3); e1 = rng.normal(size=3) * 0.3; e2 = rng.normal(size=3) * 0.3
                l.update(corner=tuple(float(x) for x in c), point1=tuple(float(x) for x in c + e1), point2=tuple(float(x) for x in c + e2))
        elif kind == "pointlight":
            l.update({"from": v(-0.7, 0.7), "power": float(rng.uniform(0.5, 3.0))})
        elif kind == "directionallight":
            l.update(direction=toward(), power=float(rng.uniform(0.3, 2.0)))
            if rng.random() < 0.5:
                l.update({"infinite": False, "from": v(-0.6, 0.6), "radius": float(rng.uniform(0.2, 1.2))})
        elif kind == "sunlight":
            l.update(direction=toward(), power=float(rng.uniform(0.3, 2.0)), angle=float(rng.choice([0.27, rng.uniform(0.5, 30.0), 85.0])), samples=int(rng.integers(1, 5)))
        else:
            l.update({"from": v(-0.7, 0.7), "radius": float(rng.choice([0.03, rng.uniform(0.05, 0.5)])), "power": float(rng.uniform(2.0, 40.0)), "samples": int(rng.integers(1, 5))})
        if rng.random() < 0.2:
            l["cast_shadows"] = False
        lights.append(l)
    return lights


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_light_mixes(seed, monkeypatch):
    """The scenes and render settings of test_random_feature_mixes with other lights: one to four of any of the five types, drawn from a
    generator of their own (the seeds of the test above keep their scenes).  Same comparison, same allowance.  Where the path tracer has
    several lights to choose from, the choice is the reference's serial counter, which the device replays: the oracle then renders
    single-threaded, in the reference's order."""
    sc, rd, w, h, base, kw = _feature_mix(seed)
    sc["lights"] = _random_lights(np.random.default_rng(9000 + seed), sc["lights"][0])
    serial = rd["integrator"] == "pathtracing" and len(sc["lights"]) > 1
    if serial:
        # the exact replay holds up to 255 integrate() calls per camera sample; past that (glossy-recursive materials four levels deep) the
        # device falls back to per-sample streams, which is no longer the reference's image (serial state).  The fuzz builder's
        # own form for serial state keeps its mixes inside that bound, and so does this one, with the same two lines.
        rd["raydepth"] = kw["raydepth"] = min(kw["raydepth"], 2 if seed % 4 == 1 else 3)
        for m in sc["materials"]:
            m.pop("additionaldepth", None)
    if seed % 2:
        monkeypatch.setenv("YAFGPU_WF_CHUNK", str([700, 1500, 4000][seed % 3]))
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film, st = yi.getFilm(w, h), yi.getRenderStats()
    assert_matches_an_oracle_render(sc, dict(rd, oracle_threads=1) if serial else rd, film, st,
                                    f"light mix {seed}: {[l['type'] for l in sc['lights']]} {kw}")


@pytest.mark.parametrize("seed", list(range(int(__import__("os").environ.get("YAFGPU_SERIAL_FUZZ_FIRST", "0")), int(__import__("os").environ.get("YAFGPU_SERIAL_FUZZ_SEEDS", "12")))))
def test_random_feature_mixes_with_serial_state(seed):
    """The random mixes again, consuming the reference's serial state (roulette stream, light counter) — with mirrors, glass and
    glossy-recursive materials a camera sample is a tree of integrate() calls whose events are replayed in the reference's depth-first
    order: the device must equal the SINGLE-THREADED oracle started from the same libc rand() state."""
    sc, rd, w, h, base, kw = _feature_mix(seed, serial=True)
    what = f"serial feature mix {seed}: {[m['type'] for m in sc['materials'][base:]]} {kw}"
    evidence = []
    for same_tree in (True, False):      # (exact-distance ties resolve by tree topology: see assert_matches_an_oracle_render)
        film, st, ofilm, ost = _render_with_rand_state(sc, rd, same_tree=same_tree)
        if (st.camera_samples, st.rays_closest, st.rays_shadow) == (ost.camera_samples, ost.rays_closest, ost.rays_shadow):
            wide = rd.get("filter_type", "box") != "box" or rd.get("AA_pixelwidth", 1.0) > 1.002      # (splats from several tiles: the plane sums round in another order)
            compare_films(film, ofilm, what, exact_weights=not wide)
            return
        # With serial state ONE query that a tree answers otherwise than the geometry does — an exact-distance tie between two
        # triangles resolved by visiting order, or a leaf the reference's walk skips over a foreign tree — shifts the light counter of
        # every sample after it.  That is the only exemption, and it has to be SHOWN: the oracle's first query (in render order) whose
        # answer over this tree differs from brute force over all triangles must be such a tie or skip, and the renders must not part
        # before the pixel it belongs to.
        evidence.append(_first_tree_artefact(sc, rd, same_tree, film, ofilm))
    for ev in evidence:
        assert ev["kind"] in ("tie", "skip", "shadow-skip"), f"{what}: differs from the single-threaded oracle and no tie explains it: {evidence}"
        assert ev["parts_at_or_after_the_query"], f"{what}: the renders part BEFORE the first tie / skip: {evidence}"
    print(f"{what}: exempt — every oracle tree has a shown artefact before the renders part: {evidence}")


def _first_tree_artefact(sc, rd, same_tree, film, ofilm):
    """the oracle's first ray query whose kd-tree answer differs from brute force, what kind of difference it is, and whether the
    device film and the oracle film agree on every pixel rendered before it (tile order = the reference's render order)"""
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    seed, skip = yi.getRandState()
    osc = po.OracleScene(sc)
    if same_tree:
        osc.set_tree(*interface.build_kdtree(sc["verts"], threads=4, device=DEVICE_TREE)[:3])
    cap = 4_000_000
    _, _, _, rays, n = osc.render_traced(dict(rd, rand_srand=seed, rand_skip=skip), 1, cap, with_shadow=True)
    assert n <= cap, "ray trace capacity"
    tris = rays[:, 9].view(np.int32)
    found = None
    for i in range(len(rays)):
        f, d, tmin, tmax = rays[i, :3], rays[i, 3:6], float(rays[i, 6]), float(rays[i, 7])
        if tris[i] == -2:
            if bool(osc.is_shadowed(f, d, tmin, tmax, use_tree=False)) != bool(rays[i, 8]):
                found = dict(kind="shadow-skip" if not rays[i, 8] else "shadow-extra", query=i)
        else:
            h, bt, t, _ = osc.intersect(f, d, tmin, tmax, use_tree=False)
            tree_hit = tris[i] >= 0
            if bool(h) != tree_hit or (h and (bt != tris[i] or np.float32(t) != rays[i, 8])):
                if h and tree_hit and np.float32(t) == rays[i, 8] and bt != tris[i]:
                    kind = "tie"            # two triangles answer the same distance: visiting order decides (kdtree_triangle.cc:782,806)
                elif h and (not tree_hit or rays[i, 8] > np.float32(t)):
                    kind = "skip"           # the walk passed over the leaf that holds the nearer hit (kdtree_triangle.cc:725-750)
                else:
                    kind = "other"
                found = dict(kind=kind, query=i, tree=(int(tris[i]), float(rays[i, 8])), brute=(int(bt) if h else -1, float(t) if h else -1.0))
        if found:
            found["pixel"] = (int(rays[i, 10]), int(rays[i, 11]))
            break
    if not found:
        return dict(kind="none", parts_at_or_after_the_query=False)
    # pixels in the reference's render order (tiles row-major, pixels row-major inside a tile); multi-pass renders revisit pixels,
    # so "before" is decided on the first pass's order: a pixel rendered before the query's pixel in EVERY pass
    ts = rd.get("tile_size", 32)
    ys, xs = np.nonzero(~np.isclose(film, ofilm, rtol=1e-4, atol=1e-6).all(axis=-1))
    x0, y0 = found["pixel"]
    x00, y00 = rd.get("xstart", 0), rd.get("ystart", 0)

    def key(x, y):
        return ((y - y00) // ts, (x - x00) // ts, y, x)
    k0 = key(x0, y0)
    # a sample lands on every pixel of its filter footprint (imagefilm.cc:124-187: filterw = AA_pixelwidth / 2, x2 gauss, x2.6 mitchell,
    # clamped to [0.501, 4]), and from the query on EVERY sample may differ (the light counter is shifted): a film pixel is "before" the
    # query only if no pixel rendered at or after it lies within the filter's reach
    fw = rd.get("AA_pixelwidth", 1.5) * 0.5 * {"gauss": 2.0, "mitchell": 2.6}.get(rd.get("filter_type", "box"), 1.0)
    reach = int(np.ceil(min(max(fw, 0.501), 4.0))) + 1
    fh, fwid = film.shape[0], film.shape[1]

    def reached_from_later(x, y):
        for qy in range(max(y - reach, y00), min(y + reach, y00 + fh - 1) + 1):
            for qx in range(max(x - reach, x00), min(x + reach, x00 + fwid - 1) + 1):
                if key(qx, qy) >= k0:
                    return True
        return False
    early = [(int(x), int(y)) for x, y in zip(xs + x00, ys + y00) if not reached_from_later(int(x), int(y))]
    if rd.get("AA_passes", 1) > 1:
        early = []      # a later pass re-renders earlier pixels after the query: order alone cannot separate them
    found["parts_at_or_after_the_query"] = not early
    found["pixels_differing_before_it"] = early[:4]
    return found


@pytest.mark.parametrize("seed", [3, 14, 25, 36, 47, 58, 69, 80])
def test_random_feature_mixes_through_the_xml_loader(seed, tmp_path):
    """The same random scenes written as scene XML and read by the C++ loader (yafaray_xml.cpp): parameter parsing,
    defaults and list order of the loader against the direct Interface calls of the test above."""
    from tests import xml_writer
    sc, rd, w, h, base, kw = _feature_mix(seed, textures=False)      # (texels in memory have no place in a scene file)
    sc = dict(sc, vnormals=None)                     # the writer emits positions and faces only
    path = str(tmp_path / f"mix{seed}.xml")
    xml_writer.write(path, sc, rd)
    yi = Interface()
    yi.loadXml(path)
    yi.render()
    film, st = yi.getFilm(w, h), yi.getRenderStats()
    direct = Interface()
    scenes.load_scene(direct, sc, rd)
    direct.render()
    dfilm, dst = direct.getFilm(w, h), direct.getRenderStats()
    assert (st.rays_closest, st.rays_shadow, st.camera_samples) == (dst.rays_closest, dst.rays_shadow, dst.camera_samples)
    if rd.get("filter_type", "box") == "box" and rd.get("AA_pixelwidth", 1.0) <= 1.002:
        assert np.array_equal(film, dfilm), "XML-loaded scene renders differently from the same scene set through the Interface"
    else:                                            # wide filters accumulate through float atomics
        np.testing.assert_allclose(film, dfilm, rtol=2e-5, atol=1e-6)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("kind", ["needles", "cluster", "scales", "sheets", "duplicates", "grid"])
def test_render_odd_geometry(kind):
    """A frame of geometry that stresses builder and traversal (tests/test_gpu_device_build.py), lit and path traced:
    the wavefront traversal with its short stack and restarts, leaves of hundreds of coincident triangles, hit-distance
    ties between duplicates."""
    from tests.test_gpu_device_build import _odd_geometry
    rng = np.random.default_rng(11)
    verts = _odd_geometry(kind, rng, 3000)
    c = verts.reshape(-1, 3).mean(axis=0); ext = float(np.abs(verts.reshape(-1, 3) - c).max())
    sc = scenes.cornell_soup(12, seed=3, res=(40, 32))
    walls = np.asarray(sc["verts"], np.float32).reshape(-1, 3, 3)[:10] * np.float32(1.6 * ext) + c.astype(np.float32)
    sc["verts"] = np.concatenate([walls, verts]).reshape(-1, 9).astype(np.float32)
    sc["tri_mat"] = np.concatenate([np.asarray(sc["tri_mat"], np.int32)[:10], rng.integers(0, 3, len(verts)).astype(np.int32)])
    sc["vnormals"] = None
    cam = sc["camera"]
    sc["camera"] = dict(cam, **{"from": tuple(float(x) for x in (c + np.array([0.0, -3.8 * 1.6 * ext, 0.0]))), "to": tuple(float(x) for x in c),
                               "up": tuple(float(x) for x in (c + np.array([0.0, -3.8 * 1.6 * ext, 1.0])))})
    sc["lights"] = [{"type": "pointlight", "from": tuple(float(x) for x in (c + np.array([0.1, -0.2, 0.9]) * 1.5 * ext)), "color": (1.0, 1.0, 1.0),
                     "power": float(8.0 * ext * ext)}]
    rd = scenes.render_settings(40, 32, 3, bounces=3, background=(0.1, 0.1, 0.2))
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.render()
    film, st = yi.getFilm(40, 32), yi.getRenderStats()
    assert st.rays_closest > 40 * 32 * 3
    assert_matches_an_oracle_render(sc, rd, film, st, f"odd geometry {kind}")
