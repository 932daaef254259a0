// TEST SUPPORT (tests/test_ies_host.py): yafgpu_scene_create on hand-made descriptors with an IES light, each the smallest one with exactly
// one fault, modelled on tests/portal_desc_cases.cpp.  Prints "case code message" per line; plain C++ against include/yafgpu.h, linked to
// the built library.
#include "yafgpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

namespace {

// The base: one triangle, one shinydiffuse material and one IES light with a 2 x 3 table.
struct Desc
{
	std::vector<float> verts = {0, 0, 0, 1, 0, 0, 0, 1, 0};
	std::vector<int32_t> tri_mat = {0};
	std::vector<yafgpu_material> mats;
	std::vector<yafgpu_light> lights;
	std::vector<float> ies = {0, 180, 0, 45, 90, 1, 2, 3, 1, 2, 3};
	yafgpu_scene_desc d;

	Desc()
	{
		std::memset(&d, 0, sizeof d);
		yafgpu_material m; std::memset(&m, 0, sizeof m);
		m.type = YAFGPU_MAT_SHINYDIFFUSE; m.c_index[0] = m.c_index[1] = -1;
		mats.push_back(m);
		yafgpu_light l; std::memset(&l, 0, sizeof l);
		l.type = YAFGPU_LIGHT_IES; l.samples = 1; l.direction[2] = 1.f; l.du[0] = -1.f; l.dv[1] = 1.f;
		l.ies_first = 0; l.ies_n_hor = 2; l.ies_n_vert = 3; l.ies_type = 1; l.ies_max_rad = 1.f / 3.f;
		lights.push_back(l);
		d.build_on_device = -1;
	}
	const yafgpu_scene_desc *finish()
	{
		d.n_tris = (int32_t)tri_mat.size(); d.verts = verts.data(); d.tri_mat = tri_mat.data();
		d.n_materials = (int32_t)mats.size(); d.materials = mats.data();
		d.n_lights = (int32_t)lights.size(); d.lights = lights.data();
		d.n_ies_floats = (int32_t)ies.size(); d.ies_tables = ies.data();
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
	run("valid_soft", [](Desc &c) { c.lights[0].type = YAFGPU_LIGHT_IES_SOFT; c.lights[0].samples = 4; });
	run("one_horizontal", [](Desc &c) { c.lights[0].ies_n_hor = 1; });
	run("one_vertical", [](Desc &c) { c.lights[0].ies_n_vert = 1; });
	run("negative_count", [](Desc &c) { c.lights[0].ies_n_vert = -3; });
	run("table_past_the_end", [](Desc &c) { c.lights[0].ies_n_vert = 4; });
	run("first_negative", [](Desc &c) { c.lights[0].ies_first = -1; });
	run("first_past_the_end", [](Desc &c) { c.lights[0].ies_first = 1; });
	run("first_overflows", [](Desc &c) { c.lights[0].ies_first = 0x7fffffff; });
	run("counts_overflow", [](Desc &c) { c.lights[0].ies_n_hor = 0x7fffffff; c.lights[0].ies_n_vert = 0x7fffffff; });
	run("no_pool", [](Desc &) {}, [](yafgpu_scene_desc &d) { d.ies_tables = nullptr; });
	run("empty_pool", [](Desc &) {}, [](yafgpu_scene_desc &d) { d.n_ies_floats = 0; });
	run("horizontal_equal", [](Desc &c) { c.ies[1] = 0.f; });
	run("horizontal_nan", [](Desc &c) { c.ies[1] = std::nanf(""); });
	run("vertical_decreasing", [](Desc &c) { c.ies[4] = 30.f; });
	run("max_rad_zero", [](Desc &c) { c.lights[0].ies_max_rad = 0.f; });
	run("max_rad_infinite", [](Desc &c) { c.lights[0].ies_max_rad = INFINITY; });
	run("max_rad_nan", [](Desc &c) { c.lights[0].ies_max_rad = std::nanf(""); });
	return 0;
}
