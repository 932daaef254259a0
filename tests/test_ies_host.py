"""IES photometric lights on the host: the parser (libyafaray_amd/csrc/yafaray_ies.cpp) and createLight's "ieslight" against the float32
restatement of tests/ies_fixture.py, bit for bit; every refusal of the parser and of yafgpu_scene_create by its message; the parser alone
in a program built with the address and undefined-behaviour sanitizers (tests/ies_parse_cases.cpp); the XML loader.  No GPU needed.

test_createlight_takes_a_file fails without the feature: createLight refused every ieslight."""
import os
import subprocess

import numpy as np
import pytest

from libyafaray_amd import Interface, interface
from tests import ies_fixture as ief
from tests.test_lights_host import F, W_COLOR, W_COS, W_DIR, W_DU, W_DV, W_POS, bits, color, light_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_IES = 14          # ies_first, ies_n_hor, ies_n_vert, ies_type, ies_max_rad (include/yafgpu.h)
NAMES = sorted(ief.SPECS)

# the fields behind the TILT= line, in the order parseIesFile reads them, as the parser's messages name them
FIELDS = ["the number of lamps", "the lumens per lamp", "the candela multiplier", "the number of vertical angles",
          "the number of horizontal angles", "the photometric type", "the units type", "the opening's width", "the opening's length",
          "the opening's height", "the ballast factor", "the ballast-lamp photometric factor", "the input watts"]


def field_of(name, k):
    """the field token k behind the TILT= line of fixture `name` belongs to"""
    _, hor, vert, _, _ = ief.SPECS[name]
    if k < len(FIELDS):
        return FIELDS[k]
    k -= len(FIELDS)
    return "the vertical angles" if k < len(vert) else "the horizontal angles" if k < len(vert) + len(hor) else "the candela values"


def cut_files(name):
    """fixture `name` cut off after every field boundary behind its TILT= line (the tilt block included): name -> (text, message)"""
    body = ief.text(name)
    head, tail = body.split("TILT=", 1)
    toks = tail.split()
    out = {}
    tilt = []
    if toks[0] == "INCLUDE":
        n = 2 + 2 * int(toks[2])
        tilt = ["the tilt block's lamp geometry", "the tilt block's pair count"] + ["the tilt block's angles and factors"] * (n - 2)
    for k in range(1, len(toks)):
        what = tilt[k - 1] if k - 1 < len(tilt) else field_of(name, k - 1 - len(tilt))
        out["%s_cut%03d" % (name, k)] = (head + "TILT=" + " ".join(toks[:k]), "the file ends before " + what)
    return out


def edited(name, **fields):
    """fixture `name` with tokens behind the TILT= line replaced: token index -> text"""
    head, tail = ief.text(name).split("TILT=NONE", 1)
    toks = tail.split()
    for k, v in fields.items():
        toks[int(k[1:])] = v
    return head + "TILT=NONE\n" + " ".join(toks) + "\n"


HUGE = "IESNA:LM-63-1995\nTILT=NONE\n1 1000 1 65535 65535 1 2 0 0 0\n1 1 100\n" + "0 " * 60
assert len(HUGE) <= 200
DAMAGED = {
    "short": ("IESNA:", "too short to be an IES file (6 bytes)"),
    "empty": ("", "too short to be an IES file (0 bytes)"),
    "wrong_header": ("IESNB:LM-63\nTILT=NONE\n", "wrong format, the first characters are not \"IESNA:\""),
    "no_tilt": ("IESNA:LM-63-1995\n[TEST] nothing else\n1 2 3\n", "no TILT= line before the end of the file"),
    "tilt_pairs_unreadable": ("IESNA:LM-63-1995\nTILT=INCLUDE\n1\nfour\n0 1 2 3\n", "cannot read the tilt block's pair count"),
    "mult_unreadable": (edited("C5x7", t2="x"), "cannot read the candela multiplier"),
    "count_unreadable": (edited("C5x7", t3="seven"), "cannot read the number of vertical angles"),
    "type_unreadable": (edited("C5x7", t5="C"), "cannot read the photometric type"),
    "width_unreadable": (edited("C5x7", t7="wide"), "cannot read the opening's width"),
    "angle_unreadable": (edited("C5x7", t14="ten"), "cannot read the vertical angles"),
    "angle_nan": (edited("C5x7", t14="nan"), "vertical angle"),
    "angle_inf": (edited("C5x7", t19="inf"), "vertical angle"),
    "angle_overflow": (edited("C5x7", t21="1e40"), "horizontal angle"),
    "candela_unreadable": (edited("C5x7", t30="-"), "cannot read the candela values"),
    "candela_overflow": (edited("C5x7", t30="1e39"), "candela value"),
    "no_horizontal": (edited("C5x7", t4="0"), "needs at least 1 horizontal and 2 vertical angles, and claims 0 and 7"),
    "one_vertical": (edited("C5x7", t3="1"), "needs at least 1 horizontal and 2 vertical angles, and claims 5 and 1"),
    "negative_count": (edited("C5x7", t3="-7"), "needs at least 1 horizontal and 2 vertical angles, and claims 5 and -7"),
    "huge_header": (HUGE, "claims 65535 horizontal and 65535 vertical angles; more than 4096 of either are refused"),
    "huge_one_side": (edited("C5x7", t4="4097"), "claims 4097 horizontal and 7 vertical angles; more than 4096 of either are refused"),
    "huge_product": (edited("C5x7", t3="4096", t4="4096"), "claims a table of 16777216 values; more than 4194304 are refused"),
    "one_horizontal_type_b": (edited("C1", t5="2"), "a single horizontal angle in a file that is not of type C"),
    "vertical_equal": (edited("C5x7", t14="0"), "the vertical angles are not strictly increasing"),
    "vertical_decreasing": (edited("C5x7", t17="20"), "the vertical angles are not strictly increasing"),
    "horizontal_equal": (edited("C5x7", t22="70"), "the horizontal angles are not strictly increasing"),
    "one_horizontal_at_180": (edited("C1", t18="180"), "the horizontal angles are not strictly increasing"),
    "all_zero": (edited("FLAT", t18="0", t19="0", t20="0", t21="0"), "no candela value above zero"),
    "all_negative": (edited("FLAT", t18="-1", t19="-1", t20="-2", t21="-1"), "no candela value above zero"),
    "tiny_maximum": (edited("FLAT", t18="1e-39", t19="0", t20="0", t21="0"), "candela value"),
}
for _n in ("C5x7", "TILT", "C1"):
    DAMAGED.update(cut_files(_n))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ies")
    paths = {n: ief.write(d, n) for n in NAMES}
    paths.update({n: ief.write(d, n, body) for n, (body, _) in DAMAGED.items()})
    return paths


def ies_light(path, **kw):
    return light_of(dict({"type": "ieslight", "file": path}, **kw))


# ---- the factory ----------------------------------------------------------------------------------------------------
def test_createlight_takes_a_file(files):
    yi, h = ies_light(files["C5x7"])
    assert h, yi.getLastError()
    assert yi.getLights().shape[0] == 1


@pytest.mark.parametrize("name", NAMES)
def test_parsed_file_and_record_bit_for_bit(files, name):
    frm, to, col, power = (0.5, -1.25, 3.0), (0.75, -1.0, 0.0), (0.9, 0.7, 0.3), 2.5
    yi, h = ies_light(files[name], **{"from": frm, "to": to, "color": color(*col), "power": power})
    assert h, yi.getLastError()
    want = ief.parsed(name)
    got = yi.getIesLight("l")
    assert got["type"] == want["type"]
    for k in ("hor", "vert", "table", "max_rad", "max_v_angle"):
        assert np.shape(got[k]) == np.shape(want[k]) and np.array_equal(bits(got[k]), bits(want[k])), (name, k, got[k], want[k])
    c = ief.consts(want, frm, to, col, power)
    rec = yi.getLights()[0]
    head = rec[:4].view(np.int32)
    assert [int(x) for x in head] == [9, 1, 1, 0]
    for w, k in ((W_DIR, "ndir"), (W_DU, "du"), (W_DV, "dv"), (W_COLOR, "color"), (W_POS, "position")):
        assert np.array_equal(bits(rec[w:w + 3]), bits(c[k])), (name, k, rec[w:w + 3], c[k])
    assert bits(rec[W_COS]) == bits(c["cos_end"])
    assert [int(x) for x in rec[W_IES:W_IES + 4].view(np.int32)] == [-1, want["hor"].size, want["vert"].size, want["type"]]
    assert bits(rec[W_IES + 4]) == bits(want["max_rad"])


def test_fixture_files_cover_what_they_are_for():
    p = {n: ief.parsed(n) for n in NAMES}
    assert p["C1"]["hor"].tolist() == [0, 180] and np.array_equal(p["C1"]["table"][0], p["C1"]["table"][1])
    assert p["FLAT"]["table"].min() == 1 == p["FLAT"]["table"].max() and p["FLAT"]["max_rad"] == 1
    assert p["C90"]["hor"][-1] == 90 and p["Cup"]["vert"].tolist() == [0, 30, 60, 90] and p["B"]["type"] == 2 and p["B"]["hor"][0] == -90
    assert p["Cup"]["max_v_angle"] == np.float32(90.0 * ief.D2R) and p["C5x7"]["max_v_angle"] == np.float32(180.0 * ief.D2R)


def test_defaults(files):
    yi, h = ies_light(files["C1"])
    assert h, yi.getLastError()
    rec = yi.getLights()[0]
    assert [int(x) for x in rec[:4].view(np.int32)] == [9, 1, 1, 0]
    assert rec[W_POS:W_POS + 3].tolist() == [0, 0, 0] and rec[W_COLOR:W_COLOR + 3].tolist() == [1, 1, 1]
    assert rec[W_DIR:W_DIR + 3].tolist() == [0, 0, 1]                  # from (0, 0, 0), to (0, 0, -1)
    assert rec[W_DU:W_DU + 3].tolist() == [-1, 0, 0] and rec[W_DV:W_DV + 3].tolist() == [0, 1, 0]      # createCs__ of (0, 0, -1)


def test_each_parameter_alone(files):
    base = ies_light(files["C5x7"])[0].getLights()[0]

    def rec_of(**kw):
        yi, h = ies_light(files["C5x7"], **kw)
        assert h, yi.getLastError()
        return yi.getLights()[0]

    def changed(rec):
        return sorted(set(np.nonzero(bits(rec) != bits(base))[0].tolist()))

    assert changed(rec_of(**{"from": (1.0, 2.0, 3.0)}))[-3:] == [W_POS, W_POS + 1, W_POS + 2]
    assert set(changed(rec_of(to=(1.0, 0.0, -1.0)))) <= set(range(W_DIR, W_COS))
    assert changed(rec_of(color=color(0.5, 0.25, 0.125))) == [W_COLOR, W_COLOR + 1, W_COLOR + 2]
    assert rec_of(power=3.0)[W_COLOR:W_COLOR + 3].tolist() == [3, 3, 3]
    assert changed(rec_of(cast_shadows=False)) == [2]
    assert changed(rec_of(samples=5)) == []                            # a Dirac light has one sample
    soft = rec_of(soft_shadows=True)
    assert changed(soft) == [0, 1] and [int(x) for x in soft[:2].view(np.int32)] == [10, 16]
    assert [int(x) for x in rec_of(soft_shadows=True, samples=5)[:2].view(np.int32)] == [10, 5]
    for k, v in (("cone_angle", 20.0), ("with_caustic", False), ("with_diffuse", False), ("photon_only", False)):
        assert changed(rec_of(**{k: v})) == [], k                      # read and unused


def test_disabled_light_leaves_the_order(files):
    yi, h = ies_light(files["C5x7"], light_enabled=False)
    assert h, yi.getLastError()
    assert yi.getLights().shape[0] == 0
    assert yi.getIesLight("l")["type"] == 1


def test_photon_only_is_refused(files):
    yi, h = ies_light(files["C5x7"], photon_only=True)
    assert not h and "photon_only" in yi.getLastError()


def test_bare_call_names_the_missing_file():
    yi, h = light_of({"type": "ieslight"})
    msg = yi.getLastError()
    assert not h and "no file given" in msg and "scope" in msg and "sunlight" in msg and "ieslight with the file it reads" in msg, msg


def test_missing_file_is_refused(tmp_path):
    path = str(tmp_path / "nothing.ies")
    yi, h = ies_light(path)
    assert not h and yi.getLastError() == 'createLight: IES file "%s": cannot open it' % path


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_damaged_file_is_refused_with_its_cause(files, name):
    yi, h = ies_light(files[name])
    msg = yi.getLastError()
    assert not h and msg.startswith('createLight: IES file "%s": ' % files[name]) and DAMAGED[name][1] in msg, msg
    assert yi.getLights().shape[0] == 0


# ---- the parser alone, under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def printout(files, tmp_path_factory):
    exe = tmp_path_factory.mktemp("ies_parse") / "ies_parse_cases"
    csrc = os.path.join(ROOT, "libyafaray_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "ies_parse_cases.cpp"), os.path.join(csrc, "yafaray_ies.cpp"), "-o", str(exe)], check=True, timeout=300)
    names = sorted(files)
    r = subprocess.run([str(exe)] + [files[n] for n in names] + [os.path.join(os.path.dirname(files["C1"]), "nothing.ies")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return {ln.split(" ", 1)[0][:-4]: ln.split(" ")[1:] for ln in r.stdout.splitlines()}


def test_standalone_parser_answers_every_file(files, printout):
    assert set(printout) == set(files) | {"nothing"}
    assert printout["nothing"][0] == "refused" and " ".join(printout["nothing"][2:]) == 'IES file "nothing.ies": cannot open it'


@pytest.mark.parametrize("name", NAMES)
def test_standalone_parser_bit_for_bit(printout, name):
    w = ief.parsed(name)
    got = printout[name]
    want = ["ok", str(w["type"]), str(w["hor"].size), str(w["vert"].size), "%08x" % bits(w["max_rad"]), "%08x" % bits(w["max_v_angle"])]
    assert got[:6] == want
    assert got[7:] == ["%08x" % b for b in bits(np.concatenate([w["hor"], w["vert"], w["table"].ravel()]))]


@pytest.mark.parametrize("name", sorted(DAMAGED))
def test_standalone_parser_refuses(printout, name):
    got = printout[name]
    assert got[0] == "refused" and DAMAGED[name][1] in " ".join(got[2:]), got
    assert " ".join(got[2:]).startswith('IES file "%s.ies": ' % name)


def test_huge_header_is_refused_without_a_large_allocation(printout):
    """65535 x 65535 angles claimed in 200 bytes: the largest single allocation while the file was parsed stays that of reading 200 bytes
    of text (a stream buffer), far below the 256 KiB of one map of 65535 floats"""
    for name in ("huge_header", "huge_one_side", "huge_product"):
        assert printout[name][0] == "refused" and int(printout[name][1]) <= 8192, printout[name][:2]


# ---- yafgpu_scene_create ------------------------------------------------------------------------------------------------
POOL = "IES light 0: its maps and table lie outside the IES table pool"
COUNT = "IES light 0: fewer than 2 horizontal or 2 vertical angles"
MAX_RAD = "IES light 0: max_rad is not finite and positive"
DESC_CASES = {
    "one_horizontal": (-2, COUNT), "one_vertical": (-2, COUNT), "negative_count": (-2, COUNT),
    "table_past_the_end": (-3, POOL), "first_negative": (-3, POOL), "first_past_the_end": (-3, POOL), "first_overflows": (-3, POOL),
    "counts_overflow": (-3, POOL), "no_pool": (-3, POOL), "empty_pool": (-3, POOL),
    "horizontal_equal": (-3, "IES light 0: its horizontal angles are not strictly increasing"),
    "horizontal_nan": (-3, "IES light 0: its horizontal angles are not strictly increasing"),
    "vertical_decreasing": (-3, "IES light 0: its vertical angles are not strictly increasing"),
    "max_rad_zero": (-3, MAX_RAD), "max_rad_infinite": (-3, MAX_RAD), "max_rad_nan": (-3, MAX_RAD),
}


@pytest.fixture(scope="module")
def desc_answers(tmp_path_factory):
    lib = interface.lib_path()
    exe = tmp_path_factory.mktemp("ies_desc") / "ies_desc_cases"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ies_desc_cases.cpp"),
                    lib, "-Wl,-rpath," + os.path.dirname(os.path.abspath(lib)), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, timeout=120, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        name, code, msg = ln.split(" ", 2)
        got[name] = (int(code), msg)
    return got


def test_every_descriptor_case_answered(desc_answers):
    assert set(desc_answers) == set(DESC_CASES) | {"valid", "valid_soft"}


@pytest.mark.parametrize("case", sorted(DESC_CASES))
def test_descriptor_refused_before_device_work(desc_answers, case):
    assert desc_answers[case] == DESC_CASES[case]


@pytest.mark.parametrize("case", ["valid", "valid_soft"])
def test_valid_descriptor_is_taken(desc_answers, case):
    """0, or the first HIP call's failure where the machine has no device"""
    code, msg = desc_answers[case]
    assert code == 0 or (code == -100 and msg.startswith("hip")), (code, msg)


# ---- XML ------------------------------------------------------------------------------------------------------------------
XML = """<?xml version="1.0"?>
<scene type="triangle">
<material name="white"><type sval="shinydiffusemat"/><color r="0.8" g="0.8" b="0.8" a="1"/><diffuse_reflect fval="1"/></material>
<light name="Downlight"><type sval="ieslight"/><file sval="%s"/><from x="0" y="0" z="2"/><to x="0" y="0" z="0"/>
  <color r="1" g="0.9" b="0.8" a="1"/><power fval="4"/><soft_shadows bval="true"/><samples ival="3"/><cone_angle fval="180"/></light>
<camera name="cam"><type sval="perspective"/><from x="0" y="-3" z="0"/><to x="0" y="0" z="0"/><up x="0" y="-3" z="1"/>
  <resx ival="16"/><resy ival="16"/><focal fval="1.2"/></camera>
<integrator name="default"><type sval="directlighting"/><caustic_type sval="none"/></integrator>
<integrator name="volintegr"><type sval="none"/></integrator>
<mesh id="1" vertices="4" faces="2" has_orco="false" has_uv="false" type="0">
  <p x="-1" y="-1" z="-1"/><p x="1" y="-1" z="-1"/><p x="1" y="1" z="-1"/><p x="-1" y="1" z="-1"/>
  <set_material sval="white"/><f a="0" b="1" c="2"/><f a="0" b="2" c="3"/>
</mesh>
<render><camera_name sval="cam"/><integrator_name sval="default"/><volintegrator_name sval="volintegr"/>
  <width ival="16"/><height ival="16"/><AA_passes ival="1"/><AA_minsamples ival="1"/>
  <AA_pixelwidth fval="1"/><filter_type sval="box"/><tile_size ival="8"/></render>
</scene>
"""


def test_xml_scene_with_an_ieslight_loads_and_a_relative_file_resolves(tmp_path):
    sub = tmp_path / "scene"
    (sub / "ies").mkdir(parents=True)
    ief.write(sub / "ies", "C5x7")
    p = sub / "downlight.xml"
    p.write_text(XML % "ies/C5x7.ies")            # relative to the XML file, not to the working directory
    assert not os.path.exists(os.path.join("ies", "C5x7.ies"))
    yi = Interface(strict=False)
    assert yi.loadXml(str(p)), yi.getLastError()
    rec = yi.getLights()
    assert [int(x) for x in rec[0, :2].view(np.int32)] == [10, 3]
    assert rec[0, W_COLOR:W_COLOR + 3].tolist() == [F(4), F(0.9) * F(4), F(0.8) * F(4)] and rec[0, W_POS + 2] == 2
    assert yi.getIesLight("Downlight")["table"].shape == (5, 7)


# ---- the flat-table render of tests/test_gpu_ies.py, on the CPU ----------------------------------------------------------
def test_flat_render_stays_under_its_caps_by_the_restatement_alone():
    """tests/test_gpu_ies.py compares the FLAT file under a tilted Dirac IES light with a point light, on the 20 x 20 plane seen from
    (0, 0, 5) at 100 x 100 pixels (the frame is 5 wide).  By the reference's formulas alone: at most 2 % of the pixels lie within the
    edge band of cos_end_ (either orientation of the image's x axis), thousands lie on either side, and inside the cone the radiance
    stays within the band the lerps' rounding allows."""
    from tests.test_gpu_ies import EDGE_BAND, TILTED
    res = 100
    xs = ((np.arange(res) + 0.5) / res - 0.5) * 5.0
    p = ief.parsed("FLAT")
    c = ief.consts(p, TILTED["from"], TILTED["to"], (1.0, 1.0, 1.0), 9.0)
    for sign in (1.0, -1.0):
        xy = np.stack(np.meshgrid(sign * xs, xs), axis=-1).reshape(-1, 2)
        pts = np.concatenate([xy, np.zeros((res * res, 1))], axis=1).astype(np.float32)
        _, _, idist_sqr, cosa, ok = ief._to_light(c, pts)
        edge = np.abs(cosa - c["cos_end"]) < EDGE_BAND
        assert edge.mean() <= 0.02 and (ok & ~edge).sum() > 1000 and (~ok & ~edge).sum() > 1000
        o = ief.illuminate(p, c, pts)
        rad = o[ok, 5].astype(np.float64) / (9.0 * idist_sqr[ok].astype(np.float64))
        assert np.abs(rad - 1).max() <= 2.0 ** -21 + 2.0 ** -23        # (the division above un-does two roundings of the colour)


# ---- the reference's compiled IesLight and IesData ------------------------------------------------------------------------
# tests/golden/ref_spot_ies_{ieee,fast}.json.gz: IesData::parseIesFile + getRadiance and IesLight made by its factory in the reference
# harness (oracle/ref_harness/ref_spot_ies.cc) on the seven files of tests/ies_fixture.py.  A row whose lookup the reference takes at or
# beyond the last entry of an angle map carries a mark and no value (the reference reads past its array there): skipped.
from tests import pin_fixture as pin                                   # noqa: E402
from tests.test_oracle_golden import FAST_ATOL, FAST_RTOL              # noqa: E402

IES_LEAVES = (("illuminate", lambda t, c, x: ief.illuminate(t, c, x)), ("illum_sample", lambda t, c, x: ief.illum_sample(t, c, x[:, :3], x[:, 3], x[:, 4])))


def file_of(p):
    return os.path.splitext(p["file"])[0]


def test_fixture_covers_every_file_in_both_modes_and_few_rows_are_marked():
    doc = pin.load("spot_ies", "ieee")
    assert doc["ies_files"] == NAMES
    assert doc["ies_sets"] == [f"ies_{n}_{mode}" for n in NAMES for mode in ("dirac", "soft")]
    for n in NAMES:
        _, _, keep = pin.leaf(doc, f"file_{n}", "radiance")
        assert len(keep) >= 500 and (~keep).mean() <= 0.05, (n, (~keep).mean())
    for name in doc["ies_sets"]:
        for fn, _ in IES_LEAVES:
            _, out, keep = pin.leaf(doc, name, fn)
            assert (~keep).mean() <= 0.05 and not out[~keep].any(), (name, fn, (~keep).mean())
            assert 0.1 <= (out[keep, 0] != 0).mean(), (name, fn)


@pytest.mark.parametrize("name", NAMES)
def test_restated_lookup_reproduces_the_reference_bit_for_bit(name):
    doc = pin.load("spot_ies", "ieee")
    inp, want, keep = pin.leaf(doc, f"file_{name}", "radiance")
    t = ief.parsed(name)
    pin.same(ief.radiance(t, inp[:, 0], inp[:, 1])[:, None], want, f"getRadiance, {name}", keep)
    # every node of both maps is among the inputs, as either angle
    for m in (t["hor"], t["vert"]):
        assert all((inp[:, 0] == a).any() and (inp[:, 1] == a).any() for a in m), name
    assert len(np.unique(want[keep])) > 50 or name == "FLAT"


def record_consts(r):
    """the constants the leaf functions read, taken from a yafgpu_light record's words"""
    return {"ndir": r[W_DIR:W_DIR + 3], "du": r[W_DU:W_DU + 3], "dv": r[W_DV:W_DV + 3], "cos_end": r[W_COS], "color": r[W_COLOR:W_COLOR + 3],
            "position": r[W_POS:W_POS + 3]}


def test_restatement_reproduces_the_reference_bit_for_bit(files):
    """tests/ies_fixture.py on the inputs of the IEEE fixture: every output word of illuminate and illumSample on the unmarked rows and the
    three flags; and the same functions fed with the words of the record createLight makes of the stored parameters and with the tables
    getIesLight() hands out, which holds colour times power, the axis, du / dv, the cone's cosine and the parsed file to the reference's
    constructor and parser at once.  The record's cosine also lies between the cosines the reference refused and took."""
    doc = pin.load("spot_ies", "ieee")
    d = os.path.dirname(files["C1"])
    for name in doc["ies_sets"]:
        p = pin.params(doc, name, d)
        t = ief.parsed(file_of(doc[name + "_params"]))
        c = ief.consts(t, p["from"], p["to"], p["color"], p["power"])
        yi, h = light_of({k: (color(*v) if k == "color" else v) for k, v in p.items()})
        assert h, (name, yi.getLastError())
        rec = yi.getLights()[0]
        soft = bool(p["soft_shadows"])
        assert doc[name + "_flags3"] == [int(not soft), 0, p["samples"]]
        assert [int(x) for x in rec[:2].view(np.int32)] == [10 if soft else 9, p["samples"] if soft else 1]
        got_t = yi.getIesLight("l")
        for fn, restated in IES_LEAVES:
            inp, want, keep = pin.leaf(doc, name, fn)
            pin.same(restated(t, c, inp), want, f"{name} {fn}", keep)
            pin.same(restated(got_t, record_consts(rec), inp), want, f"{name} {fn} from the record's words", keep)
        inp, want, keep = pin.leaf(doc, name, "illuminate")
        _, dist, _, cosa, _ = ief._to_light(record_consts(rec), inp)
        ok = want[:, 0] != 0
        refused = keep & ~ok & (dist != 0)
        if refused.any():
            assert cosa[refused].max() < rec[W_COS], name
        assert rec[W_COS] <= cosa[keep & ok].min(), name


def test_release_flag_build_of_the_reference_agrees():
    """the two builds of the reference against each other, then the restatement against the release-flag one on the rows both builds
    give a value for and agree on `ok`.  The table interpolation cancels ((1 - d) * a + d * b between entries that differ tenfold) and
    d_x, d_y are quotients of differences of angles the builds form a float step apart; where that puts the two builds further apart
    than the tolerances every release-flag fixture is compared with, the band is twice their own difference on that row ("IES
    lights", has the largest measured one)"""
    ieee, fast = pin.load("spot_ies", "ieee"), pin.load("spot_ies", "fast")
    worst = {}
    leaves = [(f"file_{n}", "radiance", n, None) for n in NAMES] + [(s, fn, file_of(ieee[s + "_params"]), r) for s in ieee["ies_sets"] for fn, r in IES_LEAVES]
    for name, fn, file, restated in leaves:
        inp, a, keep_a = pin.leaf(ieee, name, fn)
        inp_f, b, keep_b = pin.leaf(fast, name, fn)
        same_input = (inp.view(np.uint32) == inp_f.view(np.uint32)).all(axis=1)
        # (the handful of rows on the cone's rim follow each build's own cosine; the rest are the same questions)
        assert (~same_input).sum() <= 18, (name, fn, int((~same_input).sum()))
        a, b = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
        t = ief.parsed(file)
        if restated is None:
            both = keep_a & keep_b & same_input
            agree = both
            got = ief.radiance(t, inp_f[:, 0], inp_f[:, 1])[:, None].astype(np.float64)
        else:
            p = pin.params(ieee, name)
            both = keep_a & keep_b & same_input
            differ = both & (a[:, 0] != b[:, 0])
            assert differ.sum() < 0.01 * both.sum(), (name, fn, int(differ.sum()))
            agree = both & ~differ
            got = restated(t, ief.consts(t, p["from"], p["to"], p["color"], p["power"]), inp_f).astype(np.float64)
        between = np.abs(a - b)
        rel = between[agree] / np.maximum(np.abs(b[agree]), 1e-30)
        worst[fn] = max(worst.get(fn, 0.0), float(rel[np.abs(b[agree]) > 1e-3].max()))
        band = np.maximum(FAST_ATOL + FAST_RTOL * np.abs(b), 2.0 * between)
        bad = (np.abs(got - b) > band) & agree[:, None]
        assert not bad.any(), (name, fn, int(bad.sum()), np.nonzero(bad.any(axis=1))[0][:5])
        wide = ((between > FAST_ATOL + FAST_RTOL * np.abs(b)) & agree[:, None]).any(axis=1).sum()
        assert wide <= 0.02 * agree.sum(), (name, fn, int(wide))
    print("largest relative difference between the two builds of the reference, per leaf:", {k: f"{v:.3g}" for k, v in worst.items()})
