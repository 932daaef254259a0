// TEST SUPPORT (tests/test_spot_host.py): yafgpu_scene_create on hand-made descriptors with a spot light, each the smallest one with exactly
// one fault, modelled on tests/ies_desc_cases.cpp.  Prints "case code message" per line; plain C++ against include/yafgpu.h, linked to
// the built library.
#include "yafgpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

namespace {

// The base: one triangle, one shinydiffuse material and one Dirac spot light at (0, 0, 3) aimed down -z, 45 degrees, blend 0.15.
struct Desc
{
	std::vector<float> verts = {0, 0, 0, 1, 0, 0, 0, 1, 0};
	std::vector<int32_t> tri_mat = {0};
	std::vector<yafgpu_material> mats;
	std::vector<yafgpu_light> lights;
	yafgpu_scene_desc d;

	Desc()
	{
		std::memset(&d, 0, sizeof d);
		yafgpu_material m; std::memset(&m, 0, sizeof m);
		m.type = YAFGPU_MAT_SHINYDIFFUSE; m.c_index[0] = m.c_index[1] = -1;
		mats.push_back(m);
		yafgpu_light l; std::memset(&l, 0, sizeof l);
		l.type = YAFGPU_LIGHT_SPOT; l.samples = 1; l.cast_shadows = 1; l.direction[2] = 1.f; l.du[0] = -1.f; l.dv[1] = 1.f;
		l.cos_angle = 0.7078125f; l.spot_cos_start = 0.7860751f; l.spot_icos_diff = 12.777491f; l.spot_shadow_fuzzy = 1.f;
		l.color[0] = l.color[1] = l.color[2] = 1.f; l.position[2] = 3.f;
		lights.push_back(l);
		d.build_on_device = -1;
	}
	const yafgpu_scene_desc *finish()
	{
		d.n_tris = (int32_t)tri_mat.size(); d.verts = verts.data(); d.tri_mat = tri_mat.data();
		d.n_materials = (int32_t)mats.size(); d.materials = mats.data();
		d.n_lights = (int32_t)lights.size(); d.lights = lights.data();
		return &d;
	}
};

void run(const char *name, const std::function<void(Desc &)> &edit)
{
	Desc c;
	edit(c);
	c.finish();
	yafgpu_scene_t *s = nullptr;
	const int rc = yafgpu_scene_create(&c.d, &s);
	std::printf("%s %d %s\n", name, rc, rc ? yafgpu_last_error() : "ok"); std::fflush(stdout);
	if(rc == 0) yafgpu_scene_destroy(s);
}

} // namespace

int main()
{
	run("valid", [](Desc &) {});
	run("valid_soft", [](Desc &c) { c.lights[0].type = YAFGPU_LIGHT_SPOT_SOFT; c.lights[0].samples = 4; });
	run("valid_blend_zero", [](Desc &c) { c.lights[0].spot_cos_start = c.lights[0].cos_angle; c.lights[0].spot_icos_diff = INFINITY; });
	run("type_6", [](Desc &c) { c.lights[0].type = 6; });
	run("type_13", [](Desc &c) { c.lights[0].type = 13; });
	run("cos_end_nan", [](Desc &c) { c.lights[0].cos_angle = std::nanf(""); });
	run("cos_start_infinite", [](Desc &c) { c.lights[0].spot_cos_start = INFINITY; });
	run("icos_diff_nan", [](Desc &c) { c.lights[0].spot_icos_diff = std::nanf(""); });
	run("fuzzy_nan", [](Desc &c) { c.lights[0].type = YAFGPU_LIGHT_SPOT_SOFT; c.lights[0].spot_shadow_fuzzy = std::nanf(""); });
	run("axis_nan", [](Desc &c) { c.lights[0].direction[1] = std::nanf(""); });
	return 0;
}
