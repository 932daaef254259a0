"""yafgpu_scene_create's refusals for a portal light, one descriptor per fault: tests/portal_desc_cases.cpp, a plain C++ program against
include/yafgpu.h, modelled on tests/test_scene_desc_host.py.  Every fault is found on the host, before the first HIP call, so a machine
without a device answers them too."""
import os
import subprocess

import pytest

from libyafaray_amd import interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = "portal light 0: its triangles lie outside the light-geometry pool"
MAT = "portal light 0: triangle material index out of range"
CASES = {
    "no_background": (-2, "portal light 0: a portal needs a background to take its colour from"),
    "no_triangles": (-2, "portal light 0: a mesh with no triangles"),
    "pool_range_past_the_end": (-3, POOL),
    "pool_range_negative": (-3, POOL),
    "pool_range_overflows": (-3, POOL),
    "no_pool": (-3, POOL),
    "no_pool_materials": (-3, "portal light 0: no materials for the triangles of the light-geometry pool (light_tri_mat)"),
    "material_index_past_the_end": (-3, MAT),
    "material_index_negative": (-3, MAT),
    "non_finite_corner": (-3, "non-finite vertex coordinate in triangle 0 of the light-geometry pool"),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    lib = interface.lib_path()
    exe = tmp_path_factory.mktemp("portal_desc") / "portal_desc_cases"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "portal_desc_cases.cpp"),
                    lib, "-Wl,-rpath," + os.path.dirname(os.path.abspath(lib)), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, timeout=120, capture_output=True, text=True).stdout
    print(out)
    got = {}
    for ln in out.splitlines():
        name, code, msg = ln.split(" ", 2)
        got[name] = (int(code), msg)
    return got


def test_every_case_answered(answers):
    assert set(answers) == set(CASES) | {"valid"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_refused_before_device_work(answers, case):
    assert answers[case] == CASES[case]


def test_valid_descriptor_is_taken(answers):
    """0, or the first HIP call's failure where the machine has no device"""
    code, msg = answers["valid"]
    assert code == 0 or (code == -100 and msg.startswith("hip")), (code, msg)
