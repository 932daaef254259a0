"""yafgpu_scene_create's refusals, one descriptor per fault: tests/scene_desc_cases.cpp, a plain C++ program against
include/yafgpu.h linked to the built library, calls it on hand-made descriptors — the smallest ones with exactly one fault — and
prints the return code and the message of each.  Every refusal that depends on the descriptor alone is made on the host before a
scene object or any device memory exists (check_desc), so the whole table holds on a machine without a device too.

The expected codes and messages are those of the code before check_desc existed, where the second list ran after the tree build
and several uploads (there a machine without a device answered -100 to each of them).  One refusal of check_instancing has no
case: plain triangles without vertices or materials (the vertex and material loops in front of it read those arrays)."""
import os
import subprocess

import pytest

from libyafaray_amd import interface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUB = ": a sub-material index outside the table, or a mask or a blend under a %s (nesting is not built)"
PAIR = ": a glossy sub-material beside a transmitting one (recursiveRaytrace reads the union of their flags, integrator_montecarlo.cc:895-919)"
BLEND_NODE = "blend material 0: a blend with nodes needs the blend node among them, and has no bump shader"
MASK_NODE = "mask material 0: needs shader nodes and a mask node among them, and has no bump shader"
BG_LIGHT = "a background light needs a background with has_ibl, and such a background its light"
CURVE = "instanced geometry: segment 0: a curve needs two or more points inside the curve point pool"
TEXELS = "a texture's texel range lies outside the texel array"
NODES = "a material's shader nodes: more than 16 nodes, or a range outside the node array"
BUMP = "a material's bump shader: more than 16 nodes, or a range outside the node array"
ORDER = "a shader node refers to a node that is not evaluated before it (or has an unknown type; a layer needs an input)"

# materials, lights, background, instancing
EARLY = {
    "null_desc": (-1, "null argument"),
    "null_out": (-1, "null argument"),
    "no_material": (-2, "scene needs at least one material"),
    "lights_256": (-2, "more than 255 lights: the device path indexes lights with 8 bits"),
    "nan_vertex": (-3, "non-finite vertex coordinate in triangle 0"),
    "tri_mat_range": (-3, "triangle material index out of range"),
    "light_type": (-2, "light 0: unknown type"),
    "background_kind": (-2, "background: unknown kind"),
    "two_background_lights": (-2, "more than one background light"),
    "background_light_without_ibl": (-2, BG_LIGHT),
    "ibl_without_background_light": (-2, BG_LIGHT),
    "background_texture_missing": (-24, "the background's texture does not exist"),
    "background_projection": (-2, "background: unknown projection"),
    "black_background_with_light": (-2, "a constant background with a light needs a colour with energy (Pdf1D would divide by zero)"),
    "material_type": (-3, "material 0: unknown type"),
    "blend_sub_index": (-3, "blend material 0" + SUB % "blend"),
    "mask_sub_index": (-3, "mask material 0" + SUB % "mask"),
    "blend_nested": (-3, "blend material 0" + SUB % "blend"),
    "mask_nested": (-3, "mask material 0" + SUB % "mask"),
    "mask_under_blend": (-3, "blend material 0" + SUB % "blend"),
    "blend_bumped_sub": (-24, "blend material 0: a sub-material with a bump shader (BlendMaterial::initBsdf would blend two bumped frames, surface.cc:137-151)"),
    "blend_own_bump": (-24, BLEND_NODE),
    "blend_without_its_node": (-24, BLEND_NODE),
    "mask_without_its_node": (-24, MASK_NODE),
    "mask_without_nodes": (-24, MASK_NODE),
    "mask_own_bump": (-24, MASK_NODE),
    "blend_glossy_beside_transmit": (-4, "blend material 0" + PAIR),
    "mask_glossy_beside_transmit": (-4, "mask material 0" + PAIR),
    "dispersive": (-4, "material with a dispersive lobe needs recursiveRaytrace's dispersive branch, which the GPU path does not implement"),
    "glossy_transmit_not_rough_glass": (-4, "a glossy transmission lobe on a material that is not rough glass: the reflect + transmit case of recursiveRaytrace's glossy branch takes RoughGlassMaterial's two-direction sample"),
    "rough_glass_a2": (-3, "rough glass material 0: rg_a2 (alpha squared) must be positive"),
    "inst_null_segments": (-1, "instanced geometry: null segment list"),
    "inst_negative_base_count": (-3, "instanced geometry: negative base triangle count"),
    "inst_negative_curve_points": (-3, "instanced geometry: curve point pool without points"),
    "inst_curve_pool_without_points": (-1, "instanced geometry: curve point pool without points"),
    "inst_base_without_vertices": (-1, "instanced geometry: base triangles without vertices or materials"),
    "inst_base_without_materials": (-1, "instanced geometry: base triangles without vertices or materials"),
    "inst_normals_without_marks": (-1, "instanced geometry: base vertex normals without their index-0 marks"),
    "inst_segment_kind": (-3, "instanced geometry: segment 0: unknown kind"),
    "inst_curve_one_point": (-3, CURVE),
    "inst_curve_outside_pool": (-3, CURVE),
    "inst_curve_material": (-3, "instanced geometry: segment 0: curve material index out of range"),
    "inst_rows_outside_base": (-3, "instanced geometry: segment 0: rows outside the base pools"),
    "inst_rows_outside_plain": (-3, "instanced geometry: segment 0: rows outside the plain arrays"),
    "inst_too_many_triangles": (-3, "instanced geometry: more than 238609294 triangles after flattening"),
    "inst_nan_curve_point": (-3, "non-finite coordinate or extrusion scale in curve point 1"),
    "inst_base_material": (-3, "base triangle material index out of range"),
    "inst_nan_base_vertex": (-3, "non-finite vertex coordinate in base triangle 0"),
}

# textures and shader nodes: the checks that ran after the tree build and several uploads before check_desc held them
LATE = {
    "texel_range": (-24, TEXELS),
    "texel_range_background": (-24, TEXELS),
    "texture_size": (-24, TEXELS),
    "too_many_nodes": (-24, NODES),
    "node_range": (-24, NODES),
    "bump_range": (-24, BUMP),
    "bump_slot": (-24, BUMP),
    "shader_slot": (-24, "a material's shader slot names a node outside its node range"),
    "mix_refers_forward": (-24, ORDER),
    "layer_refers_forward": (-24, ORDER),
    "layer_without_input": (-24, ORDER),
    "node_type": (-24, ORDER),
    "bump_node_refers_forward": (-24, ORDER),
    "texture_mapper_without_texture": (-24, "a texture_mapper node refers to a texture that does not exist"),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    lib = interface.lib_path()
    exe = tmp_path_factory.mktemp("scene_desc") / "scene_desc_cases"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "scene_desc_cases.cpp"),
                    lib, "-Wl,-rpath," + os.path.dirname(os.path.abspath(lib)), "-o", str(exe)], check=True, timeout=300)
    out = subprocess.run([str(exe)], check=True, timeout=120, capture_output=True, text=True).stdout
    print(out)
    got = {}
    for ln in out.splitlines():
        name, code, msg = ln.split(" ", 2)
        got[name] = (int(code), msg)
    return got


def test_every_case_answered(answers):
    assert set(answers) == set(EARLY) | set(LATE) | {"valid"}


@pytest.mark.parametrize("case", sorted(EARLY))
def test_refused_before_device_work(answers, case):
    assert answers[case] == EARLY[case]


@pytest.mark.parametrize("case", sorted(LATE))
def test_refused_on_the_host_what_used_to_need_a_tree(answers, case):
    assert answers[case] == LATE[case]


def test_valid_descriptor_is_taken(answers):
    """0, or the first HIP call's failure where the machine has no device"""
    code, msg = answers["valid"]
    assert code == 0 or (code == -100 and msg.startswith("hip")), (code, msg)
