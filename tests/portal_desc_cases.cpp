// TEST SUPPORT (tests/test_portal_desc_host.py): yafgpu_scene_create on hand-made descriptors with a portal light, each the smallest one
// with exactly one fault, modelled on tests/scene_desc_cases.cpp.  Prints "case code message" per line; plain C++ against
// include/yafgpu.h, linked to the built library.
#include "yafgpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

namespace {

// The base: one triangle, one shinydiffuse material, a constant background, and one portal light over the one triangle of the
// light-geometry pool.
struct Desc
{
	std::vector<float> verts = {0, 0, 0, 1, 0, 0, 0, 1, 0};
	std::vector<int32_t> tri_mat = {0};
	std::vector<yafgpu_material> mats;
	std::vector<yafgpu_light> lights;
	std::vector<float> light_verts = {0, 0, 2, 0, 1, 2, 1, 0, 2};
	std::vector<int32_t> light_tri_mat = {0};
	yafgpu_scene_desc d;

	Desc()
	{
		std::memset(&d, 0, sizeof d);
		yafgpu_material m; std::memset(&m, 0, sizeof m);
		m.type = YAFGPU_MAT_SHINYDIFFUSE; m.c_index[0] = m.c_index[1] = -1;
		mats.push_back(m);
		yafgpu_light l; std::memset(&l, 0, sizeof l);
		l.type = YAFGPU_LIGHT_PORTAL; l.samples = 1; l.mesh_first = -1; l.mesh_count = 1; l.mesh_pool = 0; l.portal_power = 1.f;
		lights.push_back(l);
		d.background.kind = YAFGPU_BACKGROUND_CONSTANT; d.background.color[0] = d.background.color[1] = d.background.color[2] = 1.f;
		d.build_on_device = -1;
	}
	const yafgpu_scene_desc *finish()
	{
		d.n_tris = (int32_t)tri_mat.size(); d.verts = verts.data(); d.tri_mat = tri_mat.data();
		d.n_materials = (int32_t)mats.size(); d.materials = mats.data();
		d.n_lights = (int32_t)lights.size(); d.lights = lights.data();
		d.n_light_tris = (int32_t)(light_verts.size() / 9); d.light_verts = light_verts.data();
		d.light_tri_mat = light_tri_mat.empty() ? nullptr : light_tri_mat.data();
		return &d;
	}
};

void run(const char *name, const std::function<void(Desc &)> &edit, const std::function<void(yafgpu_scene_desc &)> &after = nullptr)
{
	Desc c;
	edit(c);
	c.finish();
	if(after) after(c.d);
	yafgpu_scene_t *s = nullptr;
	const int rc = yafgpu_scene_create(&c.d, &s);
	std::printf("%s %d %s\n", name, rc, rc ? yafgpu_last_error() : "ok"); std::fflush(stdout);
	if(rc == 0) yafgpu_scene_destroy(s);
}

} // namespace

int main()
{
	run("valid", [](Desc &) {});
	run("no_background", [](Desc &c) { c.d.background.kind = YAFGPU_BACKGROUND_NONE; });
	run("no_triangles", [](Desc &c) { c.lights[0].mesh_count = 0; });
	run("pool_range_past_the_end", [](Desc &c) { c.lights[0].mesh_count = 2; });
	run("pool_range_negative", [](Desc &c) { c.lights[0].mesh_pool = -1; });
	run("pool_range_overflows", [](Desc &c) { c.lights[0].mesh_pool = 0x7fffffff; });
	run("no_pool", [](Desc &) {}, [](yafgpu_scene_desc &d) { d.light_verts = nullptr; });
	run("no_pool_materials", [](Desc &) {}, [](yafgpu_scene_desc &d) { d.light_tri_mat = nullptr; });
	run("material_index_past_the_end", [](Desc &c) { c.light_tri_mat[0] = 1; });
	run("material_index_negative", [](Desc &c) { c.light_tri_mat[0] = -1; });
	run("non_finite_corner", [](Desc &c) { c.light_verts[4] = std::nanf(""); });
	return 0;
}
