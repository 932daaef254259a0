"""The oracle's film through the wide reconstruction filters against the float64 composition of tests/film_fixture.py: the sanity check of
the reference that tests/test_gpu_film_filters.py holds the device to.  The oracle adds the same float32 terms one after the other in
float32, so it must sit inside the same derived bound.  Each case also shows that the bound can see a single splat: nearly every term with
a weight is larger than twice the bound of the pixel it lands in."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import film_fixture as ff
from tests.test_cameras_host import RECORD, shoot

F = np.float32


def oracle_film(sc, rd):
    """(film, samples, colours): the oracle's render, and every camera sample coloured by the triangle the oracle's own kd-tree reports
    for its ray (the tree of the render: exact ties resolve alike), the background on a miss"""
    osc = po.OracleScene(sc)
    film, _ = osc.render(rd)
    samples = ff.sample_offsets(rd)
    frm, dr, tmin, tmax, wt = shoot(RECORD["perspective"](sc["camera"]), *samples.positions())
    assert (wt != 0).all()
    tri = np.array([(lambda hit, t, *_: t if hit else -1)(*osc.intersect(f, d, float(a), float(b), use_tree=True)) for f, d, a, b in zip(frm, dr, tmin, tmax)])
    osc.close()
    return film, samples, ff.colours_by_triangle(sc, tri)


@pytest.mark.parametrize("what,kind,width,kw", ff.HOST_CASES, ids=[c[0] for c in ff.HOST_CASES])
def test_oracle_film_within_the_bound(what, kind, width, kw):
    sc, rd = ff.box_scene(ff.FILM_CAMERA), ff.film_settings(kind, width, **kw)
    film, samples, colours = oracle_film(sc, rd)
    assert len(samples) == rd["width"] * rd["height"] * 4
    escaped = (colours == np.array(ff.BACKGROUND, F)).all(axis=1)
    assert escaped.any() and not escaped.all() and len(np.unique(colours, axis=0)) >= 3, "the frame does not mix surfaces and background"
    ref, mag, count = ff.compose(rd, samples, colours)
    bnd = ff.bound(mag, count)
    assert np.isfinite(film[..., 4]).all()
    err = np.abs(film.astype(np.float64) - ref)
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.where(err == 0, 0.0, err / bnd)))
    # sensitivity: a term that is dropped (or added twice) moves the weight channel of its pixel by |w|
    _, fy, fx, w = ff.footprint_terms(rd, samples)
    weighted = w != 0
    detectable = np.abs(w.astype(np.float64)) > 2.0 * bnd[fy, fx, 4]
    share = float(detectable[weighted].mean())
    print(f"{what}: filterw {ff.film_geometry(rd)[0]}, {len(w)} terms, {float((~weighted).mean()):.4f} of weight 0; "
          f"largest error / bound {worst:.3f}; detectable share of the weighted terms {share:.4f}, of all terms {float(detectable.mean()):.4f}")
    assert (err <= bnd).all(), f"{what}: {int((err > bnd).any(axis=-1).sum())} pixels outside the bound, largest error / bound {worst:.3g}"
    assert share >= 0.95, share


def test_geometry_and_tables():
    """the facts the cases rely on: the clamps of the half-width, negative lobes in the mitchell and lanczos tables, a box of ones"""
    assert ff.film_geometry(ff.film_settings("mitchell", 4.0))[0] == F(4.0)          # 2 * 2.6 = 5.2
    assert ff.film_geometry(ff.film_settings("lanczos", 8.0))[0] == F(4.0)
    assert ff.film_geometry(ff.film_settings("gauss", 0.3))[0] == F(0.501)           # 0.15 * 2 = 0.3
    assert ff.film_geometry(ff.film_settings("gauss", 1.5))[0] == F(1.5)
    assert ff.film_geometry(ff.film_settings("box", 2.5)) == (F(1.25), F(0.9999 * 16 / 1.25))
    tables = {k: ff.filter_table(k) for k in ff.FILTERS}
    assert all(t.dtype == F and t.shape == (16, 16) and np.isfinite(t).all() for t in tables.values())
    assert (tables["mitchell"] < 0).any() and (tables["lanczos"] < 0).any()
    assert (tables["box"] == 1).all()
    assert (tables["gauss"] >= 0).all() and (tables["gauss"] == 0).any() and tables["gauss"][0, 0] > 0.9
    for t in tables.values():
        assert np.array_equal(t, t.T)                                                # every filter is a function of dx^2 + dy^2


def test_oracle_refuses_other_cameras():
    """the oracle restates the perspective camera alone and must not render another type as one"""
    for kind in ("architect", "angular", "equirectangular"):
        with pytest.raises(ValueError):
            po.OracleScene(ff.box_scene(dict(ff.FILM_CAMERA, type=kind)))
