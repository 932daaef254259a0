"""The vertex scratchpad of the shading kernels (WfArgs::vtx_lds, vtx_keep): a resume hands the vertex it made from step to step
in LDS and a park stores only the records a later resume reads.  YAFGPU_VERTEX_LDS=0 sends every record through memory again and
stores all of them; both must render the same film, bit for bit, with the same rays — in the regime the keep-mask is narrow in
(one light with one sample, one path sample) and in every regime that has a later reader of the vertex and so keeps it whole."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes
from oracle import pyoracle as po
from tests.test_gpu_parity import compare_films
from tests.test_gpu_textures import _bumpy, _textured_box

pytestmark = pytest.mark.gpu

RES, SPP = 48, 4


def _soup(**kw):
    return scenes.cornell_soup(2000, seed=23, res=(RES, RES), sigma=0.05, **kw)


def _metric():
    return _soup(), scenes.render_settings(RES, RES, SPP, bounces=1)


def _path_samples():
    return _soup(), scenes.render_settings(RES, RES, SPP, bounces=3, path_samples=3)


def _light_samples():
    sc = _soup(n_lights=2)
    sc["lights"] = [dict(sc["lights"][0], samples=3), sc["lights"][1]]
    return sc, scenes.render_settings(RES, RES, SPP, bounces=3)


def _roulette():
    return _soup(), scenes.render_settings(RES, RES, SPP, bounces=4, russian_roulette_min_bounces=0)


def _glossy():
    return _soup(glossy_fraction=0.5), scenes.render_settings(RES, RES, SPP, bounces=3)


def _glass_and_mirror():
    sc = _soup()
    sc["materials"] = [dict(m) for m in sc["materials"]]
    sc["materials"].append({"type": "glass", "IOR": 1.5, "filter_color": (0.7, 0.95, 0.8), "transmit_filter": 0.9, "mirror_color": (1.0, 0.95, 0.9)})
    sc["materials"].append({"type": "mirror", "color": (0.9, 0.85, 0.7), "reflect": 0.9})
    tm = np.array(sc["tri_mat"], np.int32)
    free = np.arange(10, len(tm))                     # the soup triangles (the first ten are the walls)
    tm[free[0::3]] = len(sc["materials"]) - 2; tm[free[1::5]] = len(sc["materials"]) - 1
    sc["tri_mat"] = tm
    return sc, scenes.render_settings(RES, RES, SPP, bounces=3, raydepth=3)


def _bump_mapped():
    sc = _bumpy(_textured_box(n_tris=2000, specular=False))
    sc["camera"] = dict(sc["camera"], resx=RES, resy=RES)
    return sc, scenes.render_settings(RES, RES, SPP, bounces=3)


def _deep():
    return _soup(), scenes.render_settings(RES, RES, SPP, bounces=12)      # the samplers' Faure dimensions go up to 48: past the prefix staged in LDS


CASES = {
    "metric": (_metric, True),                # the narrow keep-mask: records 3, 4, 8, 9, 10 never reach memory
    "path_samples": (_path_samples, False),   # st_start_path reads the camera hit again
    "light_samples": (_light_samples, False), # an estimate of several parks (and two pairs per park): st_dl_eval on a vertex an earlier resume made
    "roulette": (_roulette, True),            # the step beside the pair is refused at roulette vertices without the replay's table, taken with it
    "glossy": (_glossy, False),
    "glass_and_mirror": (_glass_and_mirror, False),      # recursion frames, the `full` kernel
    "bump_mapped": (_bump_mapped, False),     # the general kernel: shader nodes rebuild the surface point from the parked vertex
    "deep": (_deep, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_vertex_scratchpad_on_and_off_render_the_same_film(case, monkeypatch):
    make, against_oracle = CASES[case]
    sc, rd = make()
    monkeypatch.delenv("YAFGPU_VERTEX_LDS", raising=False)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    seed, skip = yi.getRandState()
    yi.render()
    film, st = yi.getFilm(RES, RES), yi.getRenderStats()
    rays = (st.rays_closest, st.rays_shadow)
    monkeypatch.setenv("YAFGPU_VERTEX_LDS", "0")
    yi.render()
    film_off, st_off = yi.getFilm(RES, RES), yi.getRenderStats()
    assert st.camera_samples == RES * RES * SPP
    assert rays == (st_off.rays_closest, st_off.rays_shadow), f"{case}: the scratchpad changes the rays traced"
    assert rays[0] > RES * RES * SPP and rays[1] > 0
    assert np.array_equal(film, film_off), f"{case}: the scratchpad changes the film ({int((film != film_off).any(axis=-1).sum())} pixels)"
    if against_oracle:
        ofilm, ost = po.OracleScene(sc).render(dict(rd, oracle_threads=1, rand_srand=seed, rand_skip=skip))
        assert rays == (ost.rays_closest, ost.rays_shadow), f"{case}: ray counts differ from the oracle"
        compare_films(film, ofilm, f"vertex scratchpad, {case}")
