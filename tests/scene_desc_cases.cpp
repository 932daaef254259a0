// TEST SUPPORT (tests/test_scene_desc_host.py): yafgpu_scene_create on hand-made descriptors, each the smallest one with exactly one
// fault.  Prints "case code message" per line; plain C++ against include/yafgpu.h, linked to the built library.
#include "yafgpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

namespace {

// material lobe flags as the library reads them (BsdfFlags, yafgpu_shading.h)
const uint32_t kGlossy = 2u, kDispersive = 8u, kReflect = 0x10u, kTransmit = 0x20u;

// A descriptor and everything it points into.  The base: one triangle, one shinydiffuse material, no lights.
struct Desc
{
	std::vector<float> verts = {0, 0, 0, 1, 0, 0, 0, 1, 0};
	std::vector<int32_t> tri_mat = {0};
	std::vector<yafgpu_material> mats;
	std::vector<yafgpu_light> lights;
	std::vector<yafgpu_node> nodes;
	std::vector<yafgpu_texture> textures;
	std::vector<float> texels;
	// instancing: one base triangle and one segment
	std::vector<float> base_verts = {0, 0, 1, 1, 0, 1, 0, 1, 1}, base_vnormals, curve_points;
	std::vector<int32_t> base_mat = {0};
	std::vector<uint8_t> base_index0;
	std::vector<yafgpu_segment> segments;
	yafgpu_scene_desc d;

	Desc()
	{
		std::memset(&d, 0, sizeof d);
		mats.push_back(material());
		d.build_on_device = -1;
	}
	static yafgpu_material material(int type = YAFGPU_MAT_SHINYDIFFUSE)
	{
		yafgpu_material m; std::memset(&m, 0, sizeof m);
		m.type = type; m.c_index[0] = m.c_index[1] = -1;
		return m;
	}
	// two value nodes, where a node order is needed
	void add_nodes(int n = 2)
	{
		yafgpu_node v; std::memset(&v, 0, sizeof v);
		v.type = YAFGPU_NODE_VALUE; v.texture = -1; v.input1 = v.input2 = v.factor = v.input = v.upper = -1;
		nodes.assign((size_t)n, v);
	}
	// materials 1 and 2 plain, material 0 a mask or a blend over them; a mask reads node 0
	void add_pair(int type)
	{
		mats[0] = material(type); mats[0].c_index[0] = 1; mats[0].c_index[1] = 2;
		mats.push_back(material()); mats.push_back(material());
		if(type == YAFGPU_MAT_MASKED) { add_nodes(); mats[0].n_nodes = 1; }
	}
	void add_instance()
	{
		yafgpu_segment sg; std::memset(&sg, 0, sizeof sg);
		sg.kind = YAFGPU_SEGMENT_INSTANCE; sg.first = 0; sg.count = 1;
		sg.m[0] = sg.m[5] = sg.m[10] = sg.m[15] = 1.f;
		segments.push_back(sg);
	}
	void add_curve()
	{
		yafgpu_segment sg; std::memset(&sg, 0, sizeof sg);
		sg.kind = YAFGPU_SEGMENT_CURVE; sg.first = 0; sg.count = 2;
		segments.push_back(sg);
		curve_points = {0, 0, 2, 0.01f, 0.01f, 0, 0, 3, 0.01f, 0.01f};
	}
	// point the descriptor at the vectors: counts a case has set itself (non-zero) stay
	const yafgpu_scene_desc *finish()
	{
		if(!d.n_tris) d.n_tris = (int32_t)tri_mat.size();
		d.verts = verts.data(); d.tri_mat = tri_mat.data();
		if(!d.n_materials) d.n_materials = (int32_t)mats.size();
		d.materials = mats.data();
		if(!d.n_lights) d.n_lights = (int32_t)lights.size();
		d.lights = lights.empty() ? nullptr : lights.data();
		if(!d.n_nodes) d.n_nodes = (int32_t)nodes.size();
		d.nodes = nodes.empty() ? nullptr : nodes.data();
		if(!d.n_textures) d.n_textures = (int32_t)textures.size();
		d.textures = textures.empty() ? nullptr : textures.data();
		if(!d.n_texels) d.n_texels = texels.size() / 4;
		d.texels = texels.empty() ? nullptr : texels.data();
		if(!segments.empty())
		{
			yafgpu_instancing &in = d.inst;
			if(!in.n_segments) in.n_segments = (int32_t)segments.size();
			in.segments = segments.data();
			if(!in.n_base_tris) in.n_base_tris = (int32_t)base_mat.size();
			in.base_verts = base_verts.data(); in.base_mat = base_mat.data();
			in.base_vnormals = base_vnormals.empty() ? nullptr : base_vnormals.data();
			in.base_vn_index0 = base_index0.empty() ? nullptr : base_index0.data();
			if(!in.n_curve_points) in.n_curve_points = (int32_t)(curve_points.size() / 5);
			in.curve_points = curve_points.empty() ? nullptr : curve_points.data();
		}
		return &d;
	}
};

yafgpu_light light(int type) { yafgpu_light l; std::memset(&l, 0, sizeof l); l.type = type; l.samples = 1; return l; }
yafgpu_texture texture2x2() { yafgpu_texture t; std::memset(&t, 0, sizeof t); t.width = t.height = 2; return t; }

void report(const char *name, int rc) { std::printf("%s %d %s\n", name, rc, rc ? yafgpu_last_error() : "ok"); std::fflush(stdout); }

// a case edits a base descriptor; `after` edits the finished one (for the faults that are a missing pointer)
void run(const char *name, const std::function<void(Desc &)> &edit, const std::function<void(yafgpu_scene_desc &)> &after = nullptr)
{
	Desc c;
	edit(c);
	c.finish();
	if(after) after(c.d);
	yafgpu_scene_t *s = nullptr;
	const int rc = yafgpu_scene_create(&c.d, &s);
	report(name, rc);
	if(rc == 0) yafgpu_scene_destroy(s);
}

} // namespace

int main()
{
	const float nan = std::nanf("");
	{
		yafgpu_scene_t *s = nullptr; Desc c;
		report("null_desc", yafgpu_scene_create(nullptr, &s));
		report("null_out", yafgpu_scene_create(c.finish(), nullptr));
	}
	run("valid", [](Desc &) {});

	// ---- the first list: materials, lights, background
	run("no_material", [](Desc &c) { c.mats.clear(); c.tri_mat.clear(); c.verts.clear(); });
	run("lights_256", [](Desc &c) { c.lights.assign(256, light(YAFGPU_LIGHT_POINT)); });
	run("nan_vertex", [&](Desc &c) { c.verts[4] = nan; });
	run("tri_mat_range", [](Desc &c) { c.tri_mat[0] = 1; });
	run("light_type", [](Desc &c) { c.lights.push_back(light(YAFGPU_LIGHT_BACKGROUND + 1)); });
	run("background_kind", [](Desc &c) { c.d.background.kind = YAFGPU_BACKGROUND_TEXTURE + 1; });
	run("two_background_lights", [](Desc &c) {
		c.d.background.kind = YAFGPU_BACKGROUND_CONSTANT; c.d.background.has_ibl = 1; c.d.background.color[0] = 1.f;
		c.lights.assign(2, light(YAFGPU_LIGHT_BACKGROUND)); });
	run("background_light_without_ibl", [](Desc &c) { c.lights.push_back(light(YAFGPU_LIGHT_BACKGROUND)); });
	run("ibl_without_background_light", [](Desc &c) { c.d.background.kind = YAFGPU_BACKGROUND_CONSTANT; c.d.background.has_ibl = 1; c.d.background.color[0] = 1.f; });
	run("background_texture_missing", [](Desc &c) { c.d.background.kind = YAFGPU_BACKGROUND_TEXTURE; });
	run("background_projection", [](Desc &c) {
		c.d.background.kind = YAFGPU_BACKGROUND_TEXTURE; c.d.background.projection = 2;
		c.textures.push_back(texture2x2()); c.texels.assign(16, 1.f); });
	run("black_background_with_light", [](Desc &c) {
		c.d.background.kind = YAFGPU_BACKGROUND_CONSTANT; c.d.background.has_ibl = 1;
		c.lights.push_back(light(YAFGPU_LIGHT_BACKGROUND)); });
	run("material_type", [](Desc &c) { c.mats[0].type = YAFGPU_MAT_BLEND + 1; });
	run("blend_sub_index", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.mats[0].c_index[1] = 3; });
	run("mask_sub_index", [](Desc &c) { c.add_pair(YAFGPU_MAT_MASKED); c.mats[0].c_index[0] = -1; });
	run("blend_nested", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.mats[1] = Desc::material(YAFGPU_MAT_BLEND); c.mats[1].c_index[0] = c.mats[1].c_index[1] = 2; });
	run("mask_nested", [](Desc &c) {
		c.add_pair(YAFGPU_MAT_MASKED); c.mats[1] = c.mats[0]; c.mats[1].c_index[0] = c.mats[1].c_index[1] = 2; });
	run("mask_under_blend", [](Desc &c) {
		c.add_pair(YAFGPU_MAT_BLEND); c.add_nodes();
		c.mats[2] = Desc::material(YAFGPU_MAT_MASKED); c.mats[2].c_index[0] = c.mats[2].c_index[1] = 1; c.mats[2].n_nodes = 1; });
	run("blend_bumped_sub", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.add_nodes(); c.mats[2].n_bump = 1; });
	run("blend_own_bump", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.add_nodes(); c.mats[0].n_bump = 1; });
	run("blend_without_its_node", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.add_nodes(); c.mats[0].n_nodes = 1; c.mats[0].sh_diffuse = -1; });
	run("mask_without_its_node", [](Desc &c) { c.add_pair(YAFGPU_MAT_MASKED); c.mats[0].sh_diffuse = 1; });
	run("mask_without_nodes", [](Desc &c) { c.add_pair(YAFGPU_MAT_MASKED); c.nodes.clear(); });
	run("mask_own_bump", [](Desc &c) { c.add_pair(YAFGPU_MAT_MASKED); c.mats[0].n_bump = 1; });
	run("blend_glossy_beside_transmit", [](Desc &c) { c.add_pair(YAFGPU_MAT_BLEND); c.mats[1].bsdf_flags = kGlossy | kReflect; c.mats[2].bsdf_flags = kTransmit; });
	run("mask_glossy_beside_transmit", [](Desc &c) { c.add_pair(YAFGPU_MAT_MASKED); c.mats[1].bsdf_flags = kGlossy | kReflect; c.mats[2].bsdf_flags = kTransmit; });
	run("dispersive", [](Desc &c) { c.mats[0].bsdf_flags = kDispersive; });
	run("glossy_transmit_not_rough_glass", [](Desc &c) { c.mats[0].type = YAFGPU_MAT_GLOSSY; c.mats[0].bsdf_flags = kGlossy | kTransmit; });
	run("rough_glass_a2", [](Desc &c) { c.mats[0].type = YAFGPU_MAT_ROUGH_GLASS; c.mats[0].bsdf_flags = kGlossy | kReflect | kTransmit; });

	// ---- check_instancing
	run("inst_null_segments", [](Desc &c) { c.add_instance(); }, [](yafgpu_scene_desc &d) { d.inst.segments = nullptr; });
	run("inst_negative_base_count", [](Desc &c) { c.add_instance(); c.d.inst.n_base_tris = -1; });
	run("inst_negative_curve_points", [](Desc &c) { c.add_instance(); c.d.inst.n_curve_points = -1; });
	run("inst_curve_pool_without_points", [](Desc &c) { c.add_instance(); c.d.inst.n_curve_points = 2; });
	run("inst_base_without_vertices", [](Desc &c) { c.add_instance(); }, [](yafgpu_scene_desc &d) { d.inst.base_verts = nullptr; });
	run("inst_base_without_materials", [](Desc &c) { c.add_instance(); }, [](yafgpu_scene_desc &d) { d.inst.base_mat = nullptr; });
	run("inst_normals_without_marks", [](Desc &c) { c.add_instance(); c.base_vnormals.assign(9, 0.f); });
	run("inst_segment_kind", [](Desc &c) { c.add_instance(); c.segments[0].kind = YAFGPU_SEGMENT_CURVE + 1; });
	run("inst_curve_one_point", [](Desc &c) { c.add_curve(); c.segments[0].count = 1; });
	run("inst_curve_outside_pool", [](Desc &c) { c.add_curve(); c.segments[0].first = 1; });
	run("inst_curve_material", [](Desc &c) { c.add_curve(); c.segments[0].flags = 1u; });
	run("inst_rows_outside_base", [](Desc &c) { c.add_instance(); c.segments[0].count = 2; });
	run("inst_rows_outside_plain", [](Desc &c) { c.add_instance(); c.segments[0].kind = YAFGPU_SEGMENT_PLAIN; c.segments[0].first = 1; });
	run("inst_too_many_triangles", [](Desc &c) {      // a base mesh of 250 000 triangles a thousand times: 250 M rows, past INT32_MAX / 9
		c.base_verts.assign((size_t)250000 * 9, 0.f); c.base_mat.assign(250000, 0);
		c.add_instance(); c.segments[0].count = 250000; c.segments.assign(1000, c.segments[0]); });
	run("inst_nan_curve_point", [&](Desc &c) { c.add_curve(); c.curve_points[8] = nan; });
	run("inst_base_material", [](Desc &c) { c.add_instance(); c.base_mat[0] = 1; });
	run("inst_nan_base_vertex", [&](Desc &c) { c.add_instance(); c.base_verts[0] = nan; });

	// ---- the second list: textures and shader nodes (only a machine with a device could reach these while they ran after the tree build)
	run("texel_range", [](Desc &c) { c.add_nodes(); c.textures.push_back(texture2x2()); c.texels.assign(12, 1.f); });
	run("texel_range_background", [](Desc &c) {
		c.d.background.kind = YAFGPU_BACKGROUND_TEXTURE; c.textures.push_back(texture2x2()); c.textures[0].texel_first = 1u; c.texels.assign(16, 1.f); });
	run("texture_size", [](Desc &c) { c.add_nodes(); c.textures.push_back(texture2x2()); c.textures[0].width = 0; c.texels.assign(16, 1.f); });
	run("too_many_nodes", [](Desc &c) { c.add_nodes(17); c.mats[0].n_nodes = 17; });
	run("node_range", [](Desc &c) { c.add_nodes(); c.mats[0].node_first = 1; c.mats[0].n_nodes = 2; });
	run("bump_range", [](Desc &c) { c.add_nodes(); c.mats[0].bump_first = 2; c.mats[0].n_bump = 1; });
	run("bump_slot", [](Desc &c) { c.add_nodes(); c.mats[0].n_bump = 1; c.mats[0].sh_bump = 1; });
	run("shader_slot", [](Desc &c) { c.add_nodes(); c.mats[0].n_nodes = 2; c.mats[0].sh_mirror = 2; });
	run("mix_refers_forward", [](Desc &c) { c.add_nodes(); c.mats[0].n_nodes = 2; c.nodes[0].type = YAFGPU_NODE_MIX; c.nodes[0].input1 = 1; });
	run("layer_refers_forward", [](Desc &c) { c.add_nodes(); c.mats[0].n_nodes = 2; c.nodes[1].type = YAFGPU_NODE_LAYER; c.nodes[1].input = 0; c.nodes[1].upper = 1; });
	run("layer_without_input", [](Desc &c) { c.add_nodes(); c.mats[0].n_nodes = 2; c.nodes[1].type = YAFGPU_NODE_LAYER; });
	run("node_type", [](Desc &c) { c.add_nodes(); c.mats[0].n_nodes = 2; c.nodes[1].type = YAFGPU_NODE_LAYER + 1; });
	run("bump_node_refers_forward", [](Desc &c) { c.add_nodes(); c.mats[0].n_bump = 2; c.nodes[0].type = YAFGPU_NODE_MIX; c.nodes[0].factor = 0; });
	run("texture_mapper_without_texture", [](Desc &c) { c.add_nodes(); c.nodes[1].type = YAFGPU_NODE_TEXTURE_MAPPER; c.nodes[1].texture = 0; });
	return 0;
}
