"""The architect, angular and equirectangular cameras on the DEVICE, against the float32 restatement of tests/test_cameras_host.py:
rays bit for bit (probe op 7), a level architect camera against the perspective camera, whole films against an expectation composed from
restated rays and the device's own closest hits, samples without a ray (outside the angular camera's circle) through the film, the ray
counts, the serial-state replay, shards, pipelined and adaptive passes, the `window` texture coordinate — and against the reference's own compiled cameras (tests/golden/ref_cameras_ieee):
rays and `window` coordinates of all 26 ray configurations.

Frames are 24 x 16 with tiles of 7 unless stated: the aspect ratio matters, the circle cuts through pixels, the last tile is odd."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from tests import pin_fixture as pin
from tests.film_fixture import BACKGROUND, FACE_COLOURS, H, TILE, W, box_scene, box_settings, sample_offsets
from tests.test_cameras_host import (F, PROJECTIONS, RECORD, architect_record, screenproject, shoot)
from tests.test_gpu_components import exact

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """the emulated shard exchange hands device memory to torch: let torch open the GPU before the library does"""
    import torch
    torch.cuda.init()


LEVEL = {"from": (0.0, -3.0, 0.0), "to": (0.0, 0.0, 0.0), "up": (0.0, -3.0, 1.0), "resx": W, "resy": H}
TILTED = {"from": (0.2, -0.1, 0.1), "to": (0.5, 1.0, 0.4), "up": (0.3, -0.2, 1.1), "resx": W, "resy": H}
# angle / max_angle per projection: max_radius_ about 2 / 3, inside the frame's width and cutting its height; angles at which the
# orthographic and equisolid projections stay inside asin's domain in the frame's corners too (the host refuses the others)
ANGLES = {"equidistant": (90.0, 60.0), "orthographic": (50.0, 33.0), "stereographic": (90.0, 60.0), "equisolid_angle": (90.0, 60.0),
          "rectilinear": (60.0, 40.0)}


def angular(projection="equidistant", circular=True, mirrored=False, **kw):
    angle, max_angle = ANGLES[projection]
    return dict(dict(TILTED, type="angular", projection=projection, circular=circular, mirrored=mirrored, angle=angle, max_angle=max_angle), **kw)


# ---- scenes ----------------------------------------------------------------------------------------------------------
def soup_scene(cam, n_lights=2):
    sc = scenes.cornell_soup(12, seed=1, n_lights=n_lights, res=(cam["resx"], cam["resy"]))
    sc["camera"] = dict(cam)
    return sc


SOUP_VIEW = {"from": (0.0, -3.8, 0.0), "to": (0.0, 0.0, 0.0), "up": (0.0, -3.8, 1.0), "resx": W, "resy": H}
SOUP_ANGULAR = dict(SOUP_VIEW, type="angular", angle=40.0, max_angle=26.0)


def device(sc, rd, shard=None, replay=None, pipelining=None):
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    if replay is not None:
        yi.setSerialReplay(replay)
    if pipelining is not None:
        yi.setPassPipelining(pipelining)
    if shard:
        yi.setShard(*shard)
    yi.render()
    return yi.getFilm(rd["width"], rd["height"]).copy(), yi


def prepared(cam):
    yi = Interface()
    scenes.load_scene(yi, box_scene(cam), box_settings())
    yi.prepareRender()
    return yi


# ---- 1. rays, bit for bit --------------------------------------------------------------------------------------------
def ray_inputs():
    rng = np.random.default_rng(11)
    x = np.column_stack([rng.uniform(0, W, 4096), rng.uniform(0, H, 4096), rng.random(4096), rng.random(4096)]).astype(F)
    gx, gy = np.meshgrid(np.arange(0, W + 1, 3, dtype=F), np.arange(0, H + 1, 2, dtype=F))      # on pixel boundaries, the four corners among them
    grid = np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 0.25, F), np.full(gx.size, 0.75, F)])
    centre = np.array([[W / 2, H / 2, 0.5, 0.5]], F)                                              # u = v = 0: theta stays 0
    assert all(any((grid[:, 0] == a) & (grid[:, 1] == b)) for a in (0, W) for b in (0, H))
    return np.concatenate([x, grid, centre]).astype(F)


RAY_CONFIGS = [("architect level", dict(LEVEL, type="architect", focal=1.2)),
               ("architect tilted", dict(TILTED, type="architect", focal=1.2, nearClip=0.05, farClip=40.0)),
               ("architect level, lens", dict(LEVEL, type="architect", focal=1.2, aperture=0.1, dof_distance=3.0)),
               ("architect tilted, hexagon lens", dict(TILTED, type="architect", focal=1.2, aperture=0.07, dof_distance=2.0, bokeh_type="hexagon", bokeh_rotation=15.0)),
               ("equirectangular", dict(TILTED, type="equirectangular")),
               ("equirectangular, clip planes", dict(TILTED, type="equirectangular", nearClip=0.1, farClip=30.0))]
RAY_CONFIGS += [(f"angular {p} circular={c} mirrored={m}", angular(p, c, m)) for p in PROJECTIONS for c in (True, False) for m in (False, True)]


@pytest.mark.parametrize("what,cam", RAY_CONFIGS, ids=[c[0] for c in RAY_CONFIGS])
def test_rays_bit_for_bit(what, cam):
    """origin, direction, tmin, tmax and wt of probe op 7 against the restated shootRay.  architect, equirectangular and every wt: bit for
    bit on every row.  angular: a row may differ only where a double libm result of the device and of numpy narrow to neighbouring floats:
    at most 0.1 % of the rows (expected: none), each within 1e-6 per direction component (one float ulp of an angle up to pi is 2.4e-7,
    two angles enter)."""
    x = ray_inputs()
    yi = prepared(cam)
    rec = yi.getCamera("cam")
    want_rec = RECORD[cam["type"]](cam)
    assert all(np.array_equal(np.asarray(rec[k]), np.asarray(want_rec[k])) for k in want_rec), "the record is not the restated one"
    got = yi.probe(7, x, 9)
    frm, dr, tmin, tmax, wt = shoot(want_rec, x[:, 0], x[:, 1], x[:, 2], x[:, 3])
    exact(got[:, 8], wt.view(np.uint32), f"{what}: wt")
    live = wt != 0
    dead_share = float((~live).mean())
    want = np.column_stack([frm, dr, tmin, tmax]).astype(F)[live]
    g = got[live, :8]
    assert not np.isnan(g).any(), f"{what}: a live ray has a NaN"
    differ = ((g.view(np.uint32) != want.view(np.uint32)) & ~((g == 0) & (want == 0))).any(axis=1)
    share = float(differ.mean()) if len(differ) else 0.0
    worst = float(np.abs(g[differ, 3:6].astype(np.float64) - want[differ, 3:6]).max()) if differ.any() else 0.0
    print(f"{what}: {len(x)} rows, {dead_share:.3f} without a ray, {share:.5f} of the live rows not bit-exact, largest direction deviation {worst:.3g}")
    if cam["type"] != "angular":
        assert not differ.any(), f"{what}: {int(differ.sum())} rows differ; first {x[live][differ][0]}: {g[differ][0]} vs {want[differ][0]}"
    else:
        assert share <= 0.001 and worst <= 1e-6, (what, share, worst)
        assert np.array_equal(g[differ, :3].view(np.uint32), want[differ, :3].view(np.uint32))
        if cam["circular"]:
            assert 0.1 <= dead_share <= 0.9, dead_share
        else:
            assert dead_share == 0


# ---- 2. a level architect camera is the perspective camera -----------------------------------------------------------
@pytest.mark.parametrize("lens", [{}, {"aperture": 0.08, "dof_distance": 3.0, "bokeh_type": "pentagon"}], ids=["pinhole", "aperture"])
def test_level_architect_equals_perspective(lens):
    """cam_y_ is exactly (0, 0, -1): ArchitectCamera::setAxis builds PerspectiveCamera's vectors, so films and ray counts agree bit for bit"""
    cam = dict(LEVEL, focal=1.1, **lens)
    assert np.array_equal(architect_record(dict(cam, type="architect"))["cam_y"], np.array([0, 0, -1], F))
    rd = scenes.render_settings(W, H, 2, tile_size=TILE)
    films, stats = [], []
    for t in ("perspective", "architect"):
        film, yi = device(soup_scene(dict(cam, type=t)), rd)
        st = yi.getRenderStats()
        films.append(film); stats.append((st.rays_closest, st.rays_shadow, st.camera_samples))
    assert films[0][..., :3].sum() > 0
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))
    assert stats[0] == stats[1]


# ---- 3. films against a composed expectation -------------------------------------------------------------------------
def sample_positions(rd):
    """the camera samples of a render, pixel by pixel: [(film pixels the sample is added to, x, y)] — the positions of
    TiledIntegrator::renderTile (integrator_tiled.cc:386-403) and the footprint of the box filter of half-width 0.501
    (ImageFilm::addSample), enumerated as tests/test_gpu_ao.py::Restatement.camera_samples does"""
    x0, y0 = rd.get("xstart", 0), rd.get("ystart", 0)
    out = []
    for px, py, dx, dy in zip(*(sample_offsets(rd)[k] for k in (0, 1, 4, 5))):
        px, py = int(px), int(py)
        edge = lambda d: int(float(d) + float(F(0.501)) - 1.0 + (0.5 - 1.4e-11)) >= 1
        pixels = [(py + j - y0, px + i - x0) for j in range(1 + edge(dy)) for i in range(1 + edge(dx))]
        out.append(([(y, x) for y, x in pixels if y < rd["height"] and x < rd["width"]], F(F(px) + dx), F(F(py) + dy)))
    return out


def composed_film(yi, sc, rd):
    """rays from the restatement, the hit triangle from the device's own intersectRays, the colour by triangle, the background on a miss,
    black with alpha 1 for a sample without a ray -> (film sums (h, w, 5), number of live samples)"""
    rec = RECORD[sc["camera"]["type"]](sc["camera"])
    samples = sample_positions(rd)
    frm, dr, tmin, tmax, wt = shoot(rec, [s[1] for s in samples], [s[2] for s in samples])
    live = wt != 0
    colour = np.zeros((len(samples), 3), F)
    if live.any():
        tri, _, _ = yi.intersectRays(np.column_stack([frm, dr, tmin, tmax]).astype(F)[live])
        by_tri = np.array([sc["materials"][m]["color"] for m in sc["tri_mat"]], F)
        colour[live] = np.where((tri >= 0)[:, None], by_tri[np.maximum(tri, 0)], np.array(BACKGROUND, F)[None, :])
    film = np.zeros((rd["height"], rd["width"], 5), F)
    without = np.zeros((rd["height"], rd["width"]), np.int32)      # samples without a ray among those a pixel receives
    for (pixels, _, _), c, has_ray in zip(samples, colour, live):
        for y, x in pixels:
            film[y, x, :3] += c
            film[y, x, 3:] += F(1)
            without[y, x] += not has_ray
    return film, int(live.sum()), colour, live, without


FILM_CASES = [("equirectangular", dict(TILTED, type="equirectangular"), dict(spp=1)),
              ("architect tilted", dict(TILTED, type="architect", focal=0.9), dict(spp=4)),
              ("angular equidistant circular", angular(), dict(spp=4)),
              ("angular stereographic mirrored", angular("stereographic", circular=False, mirrored=True), dict(spp=4)),
              ("angular circular, window off the origin", angular(), dict(spp=4, xstart=1, ystart=1, width=13, height=9)),
              ("angular circular, two passes", angular(), dict(spp=2, AA_passes=2, AA_inc_samples=2, AA_threshold=0.0))]


@pytest.mark.parametrize("what,cam,kw", FILM_CASES, ids=[c[0] for c in FILM_CASES])
def test_film_against_composed_expectation(what, cam, kw):
    """rgb, alpha and weight sums of every pixel bit for bit, and the closest-hit ray count = the number of samples that carry a ray
    (no lights, no recursion: the camera rays are the only ones)"""
    sc, rd = box_scene(cam), box_settings(**kw)
    film, yi = device(sc, rd)
    want, n_live, colour, live, without = composed_film(yi, sc, rd)
    st = yi.getRenderStats()
    n_samples = rd["width"] * rd["height"] * (rd["AA_minsamples"] + (rd["AA_passes"] - 1) * rd.get("AA_inc_samples", 0))
    print(f"{what}: {n_samples} samples, {n_live} with a ray; {int((colour[live] == np.array(BACKGROUND, F)).all(axis=1).sum())} escape")
    assert np.array_equal(film.view(np.uint32), want.view(np.uint32)), f"{what}: {int((film != want).any(axis=-1).sum())} pixels differ"
    assert (st.rays_closest, st.rays_shadow, st.camera_samples) == (n_live, 0, n_samples)
    escaped = (colour[live] == np.array(BACKGROUND, F)).all(axis=1)
    assert escaped.any() and not escaped.all()
    if cam["type"] == "angular" and cam["circular"]:
        dead_px = without == want[..., 4]
        mixed = (without > 0) & ~dead_px
        assert 0 < n_live < n_samples and dead_px.any()
        assert not want[dead_px][:, :3].any() and (want[dead_px][:, 4] >= rd["AA_minsamples"]).all() and (want[..., 3] == want[..., 4]).all()
        assert mixed.any(), "no pixel mixes samples with and without a ray"
    if cam["type"] == "equirectangular":
        # the seam: the first and the last column look at the face behind the camera (-y, colour 1)
        px = (want[..., :3] / want[..., 4:5]).astype(F)
        behind = np.array(FACE_COLOURS[1], F)
        assert (px[H // 2 - 2:H // 2 + 2, 0] == behind).all() and (px[H // 2 - 2:H // 2 + 2, W - 1] == behind).all()


# ---- 4. a window outside the circle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("replay", [False, True])
def test_window_outside_the_circle(replay):
    """an 8 x 8 crop in the corner of a 64 x 64 circular angular camera: no sample carries a ray.  The pass runs its kernels on empty
    queues and ends: black, alpha 1, the full weight, no rays."""
    cam = dict(SOUP_VIEW, type="angular", angle=40.0, resx=64, resy=64)
    rd = scenes.render_settings(8, 8, 2, tile_size=TILE, russian_roulette_min_bounces=1)
    film, yi = device(soup_scene(cam), rd, replay=replay)
    st = yi.getRenderStats()
    assert not film[..., :3].any()
    assert np.array_equal(film[..., 3], film[..., 4]) and (film[..., 4] >= 2).all() and film[..., 4].sum() >= 2 * 64
    assert (st.rays_closest, st.rays_shadow, st.camera_samples) == (0, 0, 2 * 64)
    # the same window further in sees the scene
    film_in, yi_in = device(soup_scene(cam), dict(rd, xstart=28, ystart=28), replay=replay)
    assert film_in[..., :3].sum() > 0 and yi_in.getRenderStats().rays_closest >= 2 * 64


# ---- 5. serial state and shards --------------------------------------------------------------------------------------
def sum_of_shards(sc, rd, replay, world=2):
    """the films of `world` shards, summed, and their ray counts, summed; the light counter of the serial-state replay crosses the
    shards through an emulated exchange (as in tests/test_gpu_lights.py)"""
    import torch
    from libyafaray_amd.parallel import _DeviceFloats
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setSerialReplay(replay)
    contrib, state = {}, {"rank": 0, "k": 0, "phase": 0}

    def exchange(ptr, n):
        t = torch.as_tensor(_DeviceFloats(ptr, n), device=torch.device("cuda", 0))
        key = state["k"]; state["k"] += 1
        if state["phase"] == 0:
            contrib[(state["rank"], key)] = t.clone()
        else:
            t.copy_(sum(contrib[(r, key)] for r in range(world)))
        torch.cuda.synchronize()

    yi.setPlaneExchange(exchange)
    parts = []
    for phase in (0, 1):
        state["phase"] = phase
        for r in range(world):
            state["rank"], state["k"] = r, 0
            yi.setShard(r, world)
            yi.render()
            if phase == 1:
                st = yi.getRenderStats()
                parts.append((yi.getFilm(rd["width"], rd["height"]).copy(), (st.rays_closest, st.rays_shadow)))
    return parts, bool(contrib)


@pytest.mark.parametrize("replay", [True, False])
def test_shards_against_the_whole_frame(replay):
    """the circular angular camera into the 12-triangle Cornell soup with two area lights, path tracing with 2 bounces and roulette from
    the first, 2 spp: two shards against the whole frame.  Every pixel receives its samples from one shard's planes, except those of a
    tile's first row and column, whose left / upper neighbours may lie in the other shard's tile: there the two films meet in the
    TEST's own addition, one rounding away from the device's plane sum, as in tests/test_gpu_lights.py."""
    sc = soup_scene(SOUP_ANGULAR)
    rd = scenes.render_settings(W, H, 2, bounces=2, tile_size=TILE, russian_roulette_min_bounces=1)
    full, yi = device(sc, rd, replay=replay)
    st = yi.getRenderStats()
    dead = (full[..., :3] == 0).all(axis=-1) & (full[..., 3] == full[..., 4])
    assert full[..., :3].sum() > 0 and 0.1 < dead.mean() < 0.9
    parts, exchanged = sum_of_shards(sc, rd, replay)
    assert exchanged or not replay, "the light-counter exchange never ran"
    assert all(p[0][..., 4].sum() > 0 for p in parts)
    assert tuple(sum(p[1][k] for p in parts) for k in (0, 1)) == (st.rays_closest, st.rays_shadow)
    total = sum(p[0] for p in parts)
    interior = np.ones((H, W), bool)
    interior[::TILE, :] = False; interior[:, ::TILE] = False
    assert np.array_equal(total[..., 3:], full[..., 3:])
    assert np.array_equal(total[interior].view(np.uint32), full[interior].view(np.uint32)), "two shards do not sum to the whole frame"
    np.testing.assert_allclose(total, full, rtol=2.5e-7, atol=1e-7)


def test_replay_leaves_films_alone_where_nothing_is_serial():
    """one light, no roulette: the reference's serial state is never read, so the replay must not change a pixel — and the samples
    without a ray consume nothing of it"""
    sc = soup_scene(SOUP_ANGULAR, n_lights=1)
    rd = scenes.render_settings(W, H, 2, bounces=2, tile_size=TILE)
    on, y_on = device(sc, rd, replay=True)
    off, y_off = device(sc, rd, replay=False)
    assert on[..., :3].sum() > 0
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    a, b = y_on.getRenderStats(), y_off.getRenderStats()
    assert (a.rays_closest, a.rays_shadow) == (b.rays_closest, b.rays_shadow)


def test_pipelined_passes():
    sc = soup_scene(SOUP_ANGULAR)
    rd = scenes.render_settings(W, H, 2, bounces=2, tile_size=TILE, russian_roulette_min_bounces=1, AA_passes=3, AA_inc_samples=2, AA_threshold=0.0)
    films = [device(sc, rd, replay=False, pipelining=mode)[0] for mode in (0, 1)]
    assert films[0][..., :3].sum() > 0 and (films[0][..., 4] >= 6).all()
    assert np.array_equal(films[0].view(np.uint32), films[1].view(np.uint32))


# ---- 6. adaptive passes ----------------------------------------------------------------------------------------------
def test_adaptive_passes_leave_the_dead_region_alone():
    """AA_threshold 0.05, two passes: a pixel whose 3 x 3 neighbourhood carries no ray at all keeps the first pass's weight (nothing
    flat is resampled); noisy pixels inside the circle are sampled again"""
    sc = soup_scene(SOUP_ANGULAR)
    rd = scenes.render_settings(W, H, 2, bounces=2, tile_size=TILE, AA_passes=2, AA_inc_samples=2, AA_threshold=0.05)
    film, _ = device(sc, rd)
    first, _ = device(sc, dict(rd, AA_threshold=1.0e30))          # the second pass finds nothing to resample: the first pass alone
    rec = RECORD["angular"](SOUP_ANGULAR)
    # a pixel none of whose points lies inside the circle: its corner nearest to the centre is outside
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    nx = np.clip(W / 2, xs, xs + 1).astype(F); ny = np.clip(H / 2, ys, ys + 1).astype(F)
    outside = (shoot(rec, nx.ravel(), ny.ravel())[4] == 0).reshape(H, W) & (first[..., :3] == 0).all(axis=-1)
    m = np.pad(outside, 1, mode="edge")
    deep = np.stack([m[1 + j:1 + j + H, 1 + i:1 + i + W] for j in (-1, 0, 1) for i in (-1, 0, 1)]).all(axis=0)
    assert deep.sum() >= 20, int(deep.sum())
    assert np.array_equal(film[deep].view(np.uint32), first[deep].view(np.uint32))
    assert (film[deep][:, 4] >= 2).all() and not film[deep][:, :3].any()
    assert (film[..., 4] > first[..., 4]).any(), "nothing was resampled at all"
    assert (film[..., 4] >= first[..., 4]).all()


# ---- 7. `window` texture coordinates ---------------------------------------------------------------------------------
WINDOW_CAMERAS = [("architect", dict(TILTED, type="architect", focal=1.3, aspect_ratio=1.1)), ("angular", angular("stereographic", mirrored=True)),
                  ("equirectangular", dict(TILTED, type="equirectangular"))]


@pytest.mark.parametrize("what,cam", WINDOW_CAMERAS, ids=[c[0] for c in WINDOW_CAMERAS])
def test_window_coordinates(what, cam):
    """a texture_mapper on `window` coordinates (plain mapping, unit scale: the texture point is Camera::screenproject(p)) at 40 surface
    points (probe op 14) against the texture looked up at the restated screenproject (probe op 13), bit for bit"""
    rng = np.random.default_rng(5)
    yi = window_scene(cam, rng)
    n = 40
    p = rng.uniform(-3, 3, (n, 3)).astype(F)
    got = window_lookup(yi, p)
    s = screenproject(RECORD[cam["type"]](cam), p)
    assert np.isfinite(s).all() and len(np.unique(s[:, 0])) == n
    want = texture_at(yi, s)
    assert len(np.unique(want[:, 0])) > n // 2, "the texture does not tell the points apart"
    exact(got[:, :4], want[:, :4].view(np.uint32), f"{what}: window coordinates")


def window_scene(cam, rng):
    """one triangle whose material reads an image texture through a texture_mapper on `window` coordinates, seen by `cam`"""
    texels = rng.random((13, 17, 4)).astype(F)
    yi = Interface()
    yi.startScene(0)
    yi.paramsClearAll()
    yi.paramsSet({"type": "image", "interpolate": "bilinear", "clipping": "repeat", "color_space": "LinearRGB"})
    yi.createTextureFromMemory("t", texels)
    yi.paramsClearAll()
    yi.paramsSet({"type": "shinydiffusemat", "diffuse_shader": "map"})
    yi.paramsPushList()
    yi.paramsSet({"element": "shader_node", "type": "texture_mapper", "name": "map", "texture": "t", "texco": "window", "mapping": "plain"})
    yi.paramsEndList()
    mat = yi.createMaterial("m")
    yi.paramsClearAll()
    yi.paramsSet(cam)
    yi.createCamera("cam")
    yi.paramsClearAll()
    yi.paramsSet({"type": "directlighting", "caustic_type": "none"})
    yi.createIntegrator("default")
    yi.paramsClearAll()
    yi.paramsSet({"type": "none"})
    yi.createIntegrator("volintegr")
    yi.startGeometry()
    yi.startTriMesh(yi.getNextFreeId(), 3, 1, False, False, 0)
    for v in ((-1.0, 2.0, -1.0), (1.0, 2.0, -1.0), (0.0, 2.0, 1.0)):
        yi.addVertex(*v)
    yi.addTriangle(0, 1, 2, mat)
    yi.endTriMesh()
    yi.endGeometry()
    yi.paramsClearAll()
    yi.paramsSet({"camera_name": "cam", "integrator_name": "default", "volintegrator_name": "volintegr", "width": W, "height": H})
    assert yi.prepareRender()
    return yi


def window_lookup(yi, p):
    """probe op 14: the material's texture_mapper evaluated at surface points p, its texture point Camera::screenproject(p)"""
    sp = np.zeros((len(p), 20), F)
    sp[:, 0:3] = p
    sp[:, 3:6] = sp[:, 6:9] = (0, -1, 0)
    sp[:, 18] = np.array([0], np.uint32).view(F)[0]
    sp[:, 19] = np.array([1], np.uint32).view(F)[0]
    return yi.probe(14, sp, 5)


def texture_at(yi, s):
    """probe op 13: the texture looked up at texture points s"""
    at = np.zeros((len(s), 4), F)
    at[:, :3] = s
    at[:, 3] = np.array([0], np.uint32).view(F)[0]
    return yi.probe(13, at, 5)


# ---- 8. the reference's compiled cameras ------------------------------------------------------------------------------
PINNED = pin.load("cameras", "ieee")


@pytest.mark.parametrize("name", PINNED["sets"], ids=[PINNED[n + "_label"] for n in PINNED["sets"]])
def test_cameras_match_the_reference(name):
    """tests/golden/ref_cameras_ieee: what the reference's own ArchitectCamera, AngularCamera and EquirectangularCamera, made by their
    factories from the parameters stored there (RAY_CONFIGS, as tests/test_cameras_host.py asserts), gave.  shootRay through probe op 7
    under the exactness rule of test_rays_bit_for_bit (wt, architect and equirectangular bit for bit; an angular row may differ where a
    double libm result narrows to the neighbouring float, at most 0.1 % of the live rows, 1e-6 per direction component, origins exact);
    screenproject through the `window` coordinate (probe op 14) against the texture at the REFERENCE's screen point (probe op 13), bit
    for bit"""
    doc = PINNED
    cam = pin.params(doc, name)
    what = doc[name + "_label"]
    yi = window_scene(cam, np.random.default_rng(5))
    inp, want, _ = pin.leaf(doc, name, "shoot")
    got = yi.probe(7, inp, 9)
    exact(got[:, 8], want[:, 8], f"{what}: wt")
    live = want[:, 8] != 0
    g, w = got[live, :8], want[live, :8].view(F)
    assert not np.isnan(g).any(), f"{what}: a live ray has a NaN"
    differ = ((g.view(np.uint32) != w.view(np.uint32)) & ~((g == 0) & (w == 0))).any(axis=1)
    share = float(differ.mean())
    worst = float(np.abs(g[differ, 3:6].astype(np.float64) - w[differ, 3:6]).max()) if differ.any() else 0.0
    print(f"{what}: {len(inp)} rows, {float((~live).mean()):.3f} without a ray, {share:.5f} of the live rows not bit-exact, largest direction deviation {worst:.3g}")
    if cam["type"] != "angular":
        assert not differ.any(), f"{what}: {int(differ.sum())} rows differ; first {inp[live][differ][0]}: {g[differ][0]} vs {w[differ][0]}"
    else:
        assert share <= 0.001 and worst <= 1e-6, (what, share, worst)
        assert np.array_equal(g[differ, :3].view(np.uint32), w[differ, :3].view(np.uint32))
    p, s, _ = pin.leaf(doc, name, "project")
    got = window_lookup(yi, p)
    want = texture_at(yi, s.view(F))
    assert len(np.unique(want[:, 0])) > len(p) // 2, "the texture does not tell the points apart"
    exact(got[:, :4], want[:, :4].view(np.uint32), f"{what}: screenproject")
