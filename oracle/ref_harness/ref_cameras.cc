// TEST INFRASTRUCTURE — not product code.
//
// Reference harness for the architect, angular and equirectangular cameras.  Our driver, compiled (oracle/Makefile, target `ref`)
// against the reference's own headers and sources where they lie: camera/camera_architect.cc, camera/camera_angular.cc,
// camera/camera_equirectangular.cc on top of the component objects (which hold camera.cc and camera_perspective.cc).  Nothing of the
// reference is copied.
//
// Every camera is made by the reference's factory() from a ParamMap, and the map is stored in the document, so the factory
// conversions (degrees to radians, the focal length of each projection, the mirrored vright_, the architect's own setAxis) are pinned with
// the leaf functions.  The 26 parameter sets are those of RAY_CONFIGS in tests/test_gpu_cameras.py, in its order, on its 24 x 16 frame:
//
//   Camera::shootRay        in4 = px, py, lu, lv     out9 = from, dir, tmin, tmax, wt      (the layout of cam_ray9 in ref_components)
//   Camera::screenproject   in3 = p                  out3 = s
//
// (a sample without a ray, wt == 0, has zeros for its other outputs).  The shootRay inputs of every set, in this order: the 81 pixel-boundary
// rows (every third column, every second row, the four frame corners among them), the exact centre, for a circular angular camera points
// on its circle stepped a few floats to either side, then seeded uniform rows up to N_RAYS.  The conditions on the inputs are asserted here
// while generating: a circular angular camera leaves 10 % to 90 % of its rows without a ray and rows on both sides of its circle, every
// other camera none; no live ray carries a NaN.
//
// Output: one JSON document on stdout, floats as IEEE-754 bit patterns.  tests/golden/make_golden.py stores it as
// tests/golden/ref_cameras_{ieee,fast}.json.gz.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common/param.h"
#include "common/ray.h"
#include "camera/camera_architect.h"
#include "camera/camera_angular.h"
#include "camera/camera_equirectangular.h"

using namespace yafaray4;

static const int RESX = 24, RESY = 16;
static const int N_RAYS = 500, N_POINTS = 200;

// The inputs are formed in plain IEEE arithmetic in both builds of this driver, so that the two fixtures ask the reference the same
// questions row by row
#pragma GCC push_options
#pragma GCC optimize("no-fast-math")
static uint32_t lcg_state = 70211u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float urand() { return (float)((lcg() >> 8) * (1.0 / 16777216.0)); }
static float srand11() { return 2.f * urand() - 1.f; }
#pragma GCC pop_options
static uint32_t f2u(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
// on the bit pattern: the release-flag build of this driver folds std::isnan() to false
static bool is_nan(float f) { return (f2u(f) & 0x7fffffffu) > 0x7f800000u; }

static void require(bool ok, const char *what, const std::string &set, double value)
{
	if(ok) return;
	fprintf(stderr, "ref_cameras: %s: %s (%g)\n", set.c_str(), what, value);
	exit(2);
}

alignas(64) static unsigned char fake_env_storage[1 << 16];
static RenderEnvironment &fake_env() { return *reinterpret_cast<RenderEnvironment *>(fake_env_storage); }

// the parameters of one camera, kept twice: as the ParamMap the factory reads and as the JSON object the tests read
struct Params
{
	ParamMap pm;
	std::string json;
	void sep() { if(!json.empty()) json += ", "; }
	void str(const char *k, const char *v) { pm[k] = Parameter(std::string(v)); sep(); json += std::string("\"") + k + "\": \"" + v + "\""; }
	// (a float always with a decimal point: the ParamMap is strictly typed and a JSON reader makes "6" an int)
	void f(const char *k, float v) { pm[k] = Parameter(v); char b[64]; snprintf(b, sizeof b, "%.9g", v); sep(); json += std::string("\"") + k + "\": " + b; if(!strpbrk(b, ".eEn")) json += ".0"; }
	void i(const char *k, int v) { pm[k] = Parameter(v); char b[64]; snprintf(b, sizeof b, "\"%s\": %d", k, v); sep(); json += b; }
	void b(const char *k, bool v) { pm[k] = Parameter(v); sep(); json += std::string("\"") + k + "\": " + (v ? "true" : "false"); }
	void p(const char *k, float x, float y, float z) { pm[k] = Parameter(Point3(x, y, z)); char b[128]; snprintf(b, sizeof b, "\"%s\": [%.9g, %.9g, %.9g]", k, x, y, z); sep(); json += b; }
};

struct Doc
{
	std::string s; bool first = true;
	void key(const std::string &k) { if(!first) s += ",\n"; first = false; s += "\"" + k + "\": "; }
	void raw(const std::string &k, const std::string &v) { key(k); s += v; }
	void arr_u32(const std::string &k, const std::vector<uint32_t> &v)
	{
		key(k); s += "[";
		char b[32];
		for(size_t i = 0; i < v.size(); ++i) { snprintf(b, sizeof b, "%s%u", i ? "," : "", v[i]); s += b; }
		s += "]";
	}
};

// the two views of tests/test_gpu_cameras.py: LEVEL looks along +y with `up` straight above, TILTED is skew in every axis
static void level(Params &p) { p.p("from", 0.f, -3.f, 0.f); p.p("to", 0.f, 0.f, 0.f); p.p("up", 0.f, -3.f, 1.f); p.i("resx", RESX); p.i("resy", RESY); }
static void tilted(Params &p) { p.p("from", 0.2f, -0.1f, 0.1f); p.p("to", 0.5f, 1.f, 0.4f); p.p("up", 0.3f, -0.2f, 1.1f); p.i("resx", RESX); p.i("resy", RESY); }

struct Row { float px, py, lu, lv; };
struct Pt { float x, y, z; };

#pragma GCC push_options
#pragma GCC optimize("no-fast-math")
static Pt point_row() { Pt p; p.x = 3.f * srand11(); p.y = 3.f * srand11(); p.z = 3.f * srand11(); return p; }

// max_radius > 0: a circular angular camera with that radius and this aspect ratio (as the camera forms them; only to place the rows)
static std::vector<Row> ray_rows(float max_radius, float aspect)
{
	std::vector<Row> rows;
	for(int y = 0; y <= RESY; y += 2) for(int x = 0; x <= RESX; x += 3) rows.push_back({(float)x, (float)y, 0.25f, 0.75f});
	rows.push_back({RESX / 2.f, RESY / 2.f, 0.5f, 0.5f});
	if(max_radius > 0.f)
	{
		// sixteen points on the circle u^2 + v^2 = max_radius^2 (u = 1 - 2 px / resx, v = (2 py / resy - 1) * aspect), each stepped
		// -3 .. 3 floats in px: one step of px near 12 moves the radius by about one step of its own
		for(int k = 0; k < 16; ++k)
		{
			const double phi = (k + 0.37) * (6.283185307179586 / 16.0);
			const double u = max_radius * std::cos(phi), v = max_radius * std::sin(phi);
			float px = (float)(RESX * (1.0 - u) / 2.0);
			const float py = (float)(RESY * (v / aspect + 1.0) / 2.0);
			for(int s = 0; s < 3; ++s) px = std::nextafter(px, -1.f);
			for(int s = -3; s <= 3; ++s) { rows.push_back({px, py, urand(), urand()}); px = std::nextafter(px, 100.f); }
		}
	}
	while((int)rows.size() < N_RAYS) rows.push_back({urand() * RESX, urand() * RESY, urand(), urand()});
	return rows;
}
#pragma GCC pop_options

static void camera(Doc &j, const std::string &name, const char *label, Camera *cam, Params &pr, float max_radius)
{
	j.raw(name + "_label", std::string("\"") + label + "\"");
	j.raw(name + "_params", "{" + pr.json + "}");
	const std::vector<Row> rows = ray_rows(max_radius, (float)RESY / (float)RESX);
	std::vector<uint32_t> in, out, pin, pout;
	int dead = 0, circle_dead = 0, circle_live = 0, moved = 0;
	for(size_t k = 0; k < rows.size(); ++k)
	{
		Row r = rows[k];
		float wt = 0.f;
		Ray ray = cam->shootRay(r.px, r.py, r.lu, r.lv, wt);
		// a direction exactly across cam_z_ with the near plane through the camera makes tmin 0 / 0 (an equirectangular camera a quarter
		// turn off its axis): the project replaces that NaN on purpose ("The NaN rule"), so the fixture stays clear of it: the row
		// moves float by float towards the frame's centre, in px and py by turns (at a pole only py helps), until the reference answers with numbers
		for(int t = 0; t < 16 && wt != 0.f && is_nan(ray.tmin_); ++t)
		{
			if(t % 2 == 0) r.px = std::nextafter(r.px, RESX / 2.f); else r.py = std::nextafter(r.py, RESY / 2.f);
			ray = cam->shootRay(r.px, r.py, r.lu, r.lv, wt); ++moved;
		}
		float o[9] = {ray.from_.x_, ray.from_.y_, ray.from_.z_, ray.dir_.x_, ray.dir_.y_, ray.dir_.z_, ray.tmin_, ray.tmax_, wt};
		if(wt == 0.f) { for(int c = 0; c < 8; ++c) o[c] = 0.f; ++dead; }
		else for(int c = 0; c < 8; ++c) require(!is_nan(o[c]), "a live ray has a NaN", name, (double)k);
		if(max_radius > 0.f && k >= 82 && k < 82 + 16 * 7) { circle_dead += wt == 0.f; circle_live += wt != 0.f; }
		in.push_back(f2u(r.px)); in.push_back(f2u(r.py)); in.push_back(f2u(r.lu)); in.push_back(f2u(r.lv));
		for(int c = 0; c < 9; ++c) out.push_back(f2u(o[c]));
	}
	if(max_radius > 0.f)
	{
		require(dead * 10 >= (int)rows.size() && dead * 10 <= (int)rows.size() * 9, "a circular angular camera leaves 10 % to 90 % of the rows without a ray", name, dead);
		require(circle_dead >= 16 && circle_live >= 16, "rows on both sides of the circle", name, circle_dead);
	}
	else require(dead == 0, "this camera has a ray for every sample", name, dead);
	if(moved) fprintf(stderr, "ref_cameras: %s: %d float steps off a 0 / 0 near distance\n", name.c_str(), moved);
	for(int k = 0; k < N_POINTS; ++k)
	{
		const Pt q = point_row();
		const Point3 p(q.x, q.y, q.z);
		const Point3 s = cam->screenproject(p);
		pin.push_back(f2u(p.x_)); pin.push_back(f2u(p.y_)); pin.push_back(f2u(p.z_));
		pout.push_back(f2u(s.x_)); pout.push_back(f2u(s.y_)); pout.push_back(f2u(s.z_));
	}
	j.arr_u32(name + "_shoot_in4", in); j.arr_u32(name + "_shoot_out9", out);
	j.arr_u32(name + "_project_in3", pin); j.arr_u32(name + "_project_out3", pout);
}

int main()
{
	Doc j;
	std::string names;
	int n = 0;
	auto next = [&]() { char b[16]; snprintf(b, sizeof b, "cam%02d", n++); if(!names.empty()) names += ", "; names += std::string("\"") + b + "\""; return std::string(b); };
	{
		Params p; level(p); p.str("type", "architect"); p.f("focal", 1.2f);
		camera(j, next(), "architect level", ArchitectCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	{
		Params p; tilted(p); p.str("type", "architect"); p.f("focal", 1.2f); p.f("nearClip", 0.05f); p.f("farClip", 40.f);
		camera(j, next(), "architect tilted", ArchitectCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	{
		Params p; level(p); p.str("type", "architect"); p.f("focal", 1.2f); p.f("aperture", 0.1f); p.f("dof_distance", 3.f);
		camera(j, next(), "architect level, lens", ArchitectCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	{
		Params p; tilted(p); p.str("type", "architect"); p.f("focal", 1.2f); p.f("aperture", 0.07f); p.f("dof_distance", 2.f);
		p.str("bokeh_type", "hexagon"); p.f("bokeh_rotation", 15.f);
		camera(j, next(), "architect tilted, hexagon lens", ArchitectCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	{
		Params p; tilted(p); p.str("type", "equirectangular");
		camera(j, next(), "equirectangular", EquirectangularCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	{
		Params p; tilted(p); p.str("type", "equirectangular"); p.f("nearClip", 0.1f); p.f("farClip", 30.f);
		camera(j, next(), "equirectangular, clip planes", EquirectangularCamera::factory(p.pm, fake_env()), p, 0.f);
	}
	// angle / max_angle per projection: a circle of radius about 2 / 3, inside the frame's width and cutting its height, at angles that keep
	// the orthographic and equisolid projections inside asin's domain in the frame's corners too
	const char *projection[5] = {"equidistant", "orthographic", "stereographic", "equisolid_angle", "rectilinear"};
	const float angle[5] = {90.f, 50.f, 90.f, 90.f, 60.f}, max_angle[5] = {60.f, 33.f, 60.f, 60.f, 40.f};
	for(int k = 0; k < 5; ++k) for(int circular = 1; circular >= 0; --circular) for(int mirrored = 0; mirrored <= 1; ++mirrored)
	{
		Params p; tilted(p); p.str("type", "angular"); p.str("projection", projection[k]); p.b("circular", circular); p.b("mirrored", mirrored);
		p.f("angle", angle[k]); p.f("max_angle", max_angle[k]);
		char label[96]; snprintf(label, sizeof label, "angular %s circular=%s mirrored=%s", projection[k], circular ? "True" : "False", mirrored ? "True" : "False");
		// max_radius_ as the factory and the constructor form it (double degrees to float radians, a float quotient)
		const float a = (float)((double)angle[k] * M_PI / 180.f), m = (float)((double)max_angle[k] * M_PI / 180.f);
		camera(j, next(), label, AngularCamera::factory(p.pm, fake_env()), p, circular ? m / a : 0.f);
	}
	j.raw("sets", "[" + names + "]");
	printf("{\n%s\n}\n", j.s.c_str());
	return 0;
}
