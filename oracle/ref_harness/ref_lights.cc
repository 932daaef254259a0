// TEST INFRASTRUCTURE — not product code.
//
// Reference harness for the directional, sun and sphere lights.  Our driver, compiled (oracle/Makefile, target `ref`)
// against the reference's own headers and sources where they lie: light/light_directional.cc, light/light_sun.cc,
// light/light_sphere.cc on top of the component objects.  Nothing of the reference is copied.
//
// Every light is made by the reference's factory() from a ParamMap, and the map is stored in the document, so the
// factory conversions (degrees to cosine, colour times power, the squared radius and its epsilon) are pinned with the
// leaf functions:
//
//   DirectionalLight::illuminate   in3  = p                 out8 = ok, wi.dir_, wi.tmax_, colour
//   SunLight::illumSample          in2  = s_1, s_2          out9 = ok, wi.dir_, wi.tmax_, s.pdf_, s.col_
//   SunLight::intersect            in3  = ray.dir_          out6 = ok, t, ipdf, colour
//   SphereLight::illumSample       in5  = p, s_1, s_2       out9 = ok, wi.dir_, wi.tmax_, s.pdf_, s.col_
//   diracLight(), canIntersect(), nSamples() of each light  flags3
//
// (the outputs of a refused call are zeros).  N_IN seeded inputs per parameter set.  The conditions on the inputs — how many
// points a finite directional light accepts, how many directions a sun accepts, how many points lie inside a sphere
// light and just inside / outside its surface — are asserted here while generating.
//
// Scene::getSceneBound and Scene::getObject stay unresolved: only the lights' init() (photon emission) calls them, and
// nothing here does.
//
// Output: one JSON document on stdout, floats as IEEE-754 bit patterns.  tests/golden/make_golden.py stores it as
// tests/golden/ref_lights_{ieee,fast}.json.gz.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common/param.h"
#include "common/surface.h"
#include "common/scene.h"
#include "common/ray.h"
#include "light/light_directional.h"
#include "light/light_sun.h"
#include "light/light_sphere.h"

using namespace yafaray4;

static const int N_IN = 2000;

static uint32_t lcg_state = 20211u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
static float urand() { return (float)((lcg() >> 8) * (1.0 / 16777216.0)); }
static float srand11() { return 2.f * urand() - 1.f; }
static uint32_t f2u(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }

static Vec3 rand_unit()
{
	for(;;)
	{
		Vec3 v(srand11(), srand11(), srand11());
		float l = v.lengthSqr();
		if(l > 0.01f && l < 1.f) { v.normalize(); return v; }
	}
}

static void require(bool ok, const char *what, const std::string &set, double value)
{
	if(ok) return;
	fprintf(stderr, "ref_lights: %s: %s (%g)\n", set.c_str(), what, value);
	exit(2);
}

alignas(64) static unsigned char fake_env_storage[1 << 16];
static RenderEnvironment &fake_env() { return *reinterpret_cast<RenderEnvironment *>(fake_env_storage); }

static void pushv(std::vector<uint32_t> &o, const Vec3 &v) { o.push_back(f2u(v.x_)); o.push_back(f2u(v.y_)); o.push_back(f2u(v.z_)); }
static void pushp(std::vector<uint32_t> &o, const Point3 &v) { o.push_back(f2u(v.x_)); o.push_back(f2u(v.y_)); o.push_back(f2u(v.z_)); }
static void pushc(std::vector<uint32_t> &o, const Rgb &c) { o.push_back(f2u(c.r_)); o.push_back(f2u(c.g_)); o.push_back(f2u(c.b_)); }

// the parameters of one light, kept twice: as the ParamMap the factory reads and as the JSON object the tests read
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
	void c(const char *k, float r, float g, float bl) { pm[k] = Parameter(Rgba(r, g, bl, 1.f)); char b[128]; snprintf(b, sizeof b, "\"%s\": [%.9g, %.9g, %.9g]", k, r, g, bl); sep(); json += b; }
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

static void surface_at(SurfacePoint &sp, const Point3 &p)
{
	sp.p_ = p; sp.n_ = sp.ng_ = Vec3(0, 0, 1);
	sp.material_ = nullptr; sp.light_ = nullptr; sp.object_ = nullptr; sp.origin_ = nullptr; sp.ray_ = nullptr;
}

static void flags(Doc &j, const std::string &name, const Light *l)
{
	j.arr_u32(name + "_flags3", {l->diracLight() ? 1u : 0u, l->canIntersect() ? 1u : 0u, (uint32_t)l->nSamples()});
}

static void directional(Doc &j, const std::string &name, Params &pr, bool finite, const Point3 &from, float radius)
{
	Light *l = DirectionalLight::factory(pr.pm, fake_env());
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	std::vector<uint32_t> in, out;
	int accepted = 0;
	for(int k = 0; k < N_IN; ++k)
	{
		// finite: points in a box of 1.6 radii around `from`, both sides of it along the direction
		const float ext = finite ? 1.6f * radius : 5.f;
		Point3 p(from.x_ + srand11() * ext, from.y_ + srand11() * ext, from.z_ + srand11() * ext);
		SurfacePoint sp; surface_at(sp, p);
		Ray wi; Rgb col(0.f);
		bool ok = l->illuminate(sp, col, wi);
		if(!ok) { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; col = Rgb(0.f); }
		accepted += ok;
		pushp(in, p);
		out.push_back(f2u(ok ? 1.f : 0.f)); pushv(out, wi.dir_); out.push_back(f2u(wi.tmax_)); pushc(out, col);
	}
	if(finite) require(accepted >= N_IN / 10 && accepted <= N_IN * 9 / 10, "finite directional light must accept 10 % to 90 % of the points", name, accepted);
	else require(accepted == N_IN, "an infinite directional light accepts every point", name, accepted);
	j.arr_u32(name + "_illuminate_in3", in); j.arr_u32(name + "_illuminate_out8", out);
}

static void sun(Doc &j, const std::string &name, Params &pr, const Vec3 &axis_given, float angle_deg)
{
	Light *l = SunLight::factory(pr.pm, fake_env());
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	std::vector<uint32_t> in, out, iin, iout;
	for(int k = 0; k < N_IN; ++k)
	{
		LSample ls; ls.s_1_ = urand(); ls.s_2_ = urand();
		if(k % 97 == 0) ls.s_2_ = (k % 2) ? 0.f : 1.f;         // the cone's axis and its rim
		SurfacePoint sp; surface_at(sp, Point3(srand11(), srand11(), srand11()));
		Ray wi; ls.pdf_ = 0.f; ls.col_ = Rgb(0.f);
		bool ok = l->illumSample(sp, ls, wi);
		if(!ok) { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; ls.pdf_ = 0.f; ls.col_ = Rgb(0.f); }
		in.push_back(f2u(ls.s_1_)); in.push_back(f2u(ls.s_2_));
		out.push_back(f2u(ok ? 1.f : 0.f)); pushv(out, wi.dir_); out.push_back(f2u(wi.tmax_)); out.push_back(f2u(ls.pdf_)); pushc(out, ls.col_);
	}
	// directions around the axis, the spread scaled to the cone: the tangent offset is uniform in a disk of 1.5 cone radii
	Vec3 axis = axis_given; axis.normalize();
	Vec3 u, v; createCs__(axis, u, v);
	const double tan_cone = std::tan((double)angle_deg * 3.14159265358979323846 / 180.0);
	int accepted = 0;
	for(int k = 0; k < N_IN; ++k)
	{
		const float r = 1.5f * (float)tan_cone * std::sqrt(urand()), phi = 6.2831853f * urand();
		Vec3 d = axis + u * (r * std::cos(phi)) + v * (r * std::sin(phi));
		d.normalize();
		if(k % 101 == 0) d = rand_unit();
		Ray ray(Point3(srand11(), srand11(), srand11()), d);
		float t = 0.f, ipdf = 0.f; Rgb col(0.f);
		bool ok = l->intersect(ray, t, col, ipdf);
		if(!ok) { t = 0.f; ipdf = 0.f; col = Rgb(0.f); }
		accepted += ok;
		pushv(iin, d);
		iout.push_back(f2u(ok ? 1.f : 0.f)); iout.push_back(f2u(t)); iout.push_back(f2u(ipdf)); pushc(iout, col);
	}
	require(accepted >= N_IN / 10 && accepted <= N_IN * 9 / 10, "a sun must accept 10 % to 90 % of the intersect directions", name, accepted);
	j.arr_u32(name + "_illum_sample_in2", in); j.arr_u32(name + "_illum_sample_out9", out);
	j.arr_u32(name + "_intersect_in3", iin); j.arr_u32(name + "_intersect_out6", iout);
}

static void sphere(Doc &j, const std::string &name, Params &pr, const Point3 &c, float radius)
{
	Light *l = SphereLight::factory(pr.pm, fake_env());
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	std::vector<uint32_t> in, out;
	int inside = 0, near_out = 0, near_in = 0, refused_inside = 0;
	for(int k = 0; k < N_IN; ++k)
	{
		// where the point lies, in radii from the centre: a shell just outside (within 1 %), one just inside (within 3 %), well
		// inside, close by, far away.  The outer shell starts 0.05 % above the surface: cos_alpha = sqrt(1 - r^2 / d^2) loses
		// 1 / (2 (1 - r^2 / d^2)) of its precision there, 1000 float epsilons at 0.05 % (6e-5, inside the tolerance the release-flag
		// fixture is compared with) and all of it on the surface itself, where the two builds of the reference have no digit in common
		float rho;
		switch(k % 8)
		{
			case 0: rho = 1.0005f + 0.0094f * urand(); break;
			case 1: rho = 1.f - 0.0299f * urand(); break;
			case 2: rho = 0.9f * urand(); break;
			case 3: rho = 1.f + 0.3f * urand(); break;
			default: rho = 1.f + 12.f * urand() * urand(); break;
		}
		Point3 p = c + (rho * radius) * rand_unit();
		const double dist = std::sqrt((double)(p.x_ - c.x_) * (p.x_ - c.x_) + (double)(p.y_ - c.y_) * (p.y_ - c.y_) + (double)(p.z_ - c.z_) * (p.z_ - c.z_)) / (double)radius;
		inside += dist < 1.0; near_out += dist > 1.0 && dist < 1.01; near_in += dist < 1.0 && dist > 0.97;
		SurfacePoint sp; surface_at(sp, p);
		LSample ls; ls.s_1_ = urand(); ls.s_2_ = urand(); ls.pdf_ = 0.f; ls.col_ = Rgb(0.f);
		if(k % 89 == 0) ls.s_2_ = 1.f;                         // the cone's rim: the tangential branch of the sphere intersection
		Ray wi; wi.from_ = p;
		bool ok = l->illumSample(sp, ls, wi);
		if(!ok) { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; ls.pdf_ = 0.f; ls.col_ = Rgb(0.f); }
		refused_inside += (!ok && dist < 1.0);
		pushp(in, p); in.push_back(f2u(ls.s_1_)); in.push_back(f2u(ls.s_2_));
		out.push_back(f2u(ok ? 1.f : 0.f)); pushv(out, wi.dir_); out.push_back(f2u(wi.tmax_)); out.push_back(f2u(ls.pdf_)); pushc(out, ls.col_);
	}
	require(inside >= 100 && refused_inside >= 100, "at least 100 points inside the sphere, refused", name, refused_inside);
	require(near_out >= 100, "at least 100 points within 1 % of the radius outside", name, near_out);
	require(near_in >= 100, "at least 100 points within 3 % of the radius inside", name, near_in);
	j.arr_u32(name + "_illum_sample_in5", in); j.arr_u32(name + "_illum_sample_out9", out);
}

int main()
{
	Doc j;
	std::string names;
	auto add = [&](const char *n) { if(!names.empty()) names += ", "; names += std::string("\"") + n + "\""; };
	{
		Params p; p.str("type", "directionallight"); p.p("direction", 0.3f, -0.4f, 1.2f); p.c("color", 0.9f, 0.5f, 0.3f); p.f("power", 2.5f);
		add("dir_inf_a"); directional(j, "dir_inf_a", p, false, Point3(0.f), 1.f);
	}
	{	// infinite stated, `from` and `radius` given and not read (light_directional.cc:142)
		Params p; p.str("type", "directionallight"); p.p("direction", -2.f, 0.5f, -0.25f); p.c("color", 1.f, 1.f, 0.8f); p.f("power", 0.75f);
		p.b("infinite", true); p.p("from", 1.f, 2.f, 3.f); p.f("radius", 0.5f); p.b("cast_shadows", false);
		add("dir_inf_b"); directional(j, "dir_inf_b", p, false, Point3(0.f), 1.f);
	}
	{
		Params p; p.str("type", "directionallight"); p.p("direction", -0.2f, 0.5f, 1.f); p.c("color", 0.6f, 0.7f, 1.f); p.f("power", 4.f);
		p.b("infinite", false); p.p("from", 0.5f, -0.5f, 4.f); p.f("radius", 2.5f);
		add("dir_fin_a"); directional(j, "dir_fin_a", p, true, Point3(0.5f, -0.5f, 4.f), 2.5f);
	}
	{
		Params p; p.str("type", "directionallight"); p.p("direction", 0.f, 0.f, -3.f); p.c("color", 1.f, 0.25f, 0.5f); p.f("power", 1.5f);
		p.b("infinite", false); p.p("from", -1.25f, 0.75f, -0.5f); p.f("radius", 0.3f);
		add("dir_fin_b"); directional(j, "dir_fin_b", p, true, Point3(-1.25f, 0.75f, -0.5f), 0.3f);
	}
	const float sun_angle[3] = {0.5f, 6.f, 40.f};
	const float sun_dir[3][3] = {{0.6f, 0.2f, 0.9f}, {0.f, 0.f, -2.f}, {-0.3f, 0.8f, 0.1f}};
	const char *sun_name[3] = {"sun_0_5", "sun_6", "sun_40"};
	for(int k = 0; k < 3; ++k)
	{
		Params p; p.str("type", "sunlight"); p.p("direction", sun_dir[k][0], sun_dir[k][1], sun_dir[k][2]);
		p.c("color", 1.f, 0.8f - 0.1f * k, 0.6f); p.f("power", 1.5f + k); p.f("angle", sun_angle[k]); p.i("samples", 2 + 3 * k);
		add(sun_name[k]); sun(j, sun_name[k], p, Vec3(sun_dir[k][0], sun_dir[k][1], sun_dir[k][2]), sun_angle[k]);
	}
	const float sph_radius[3] = {0.05f, 0.4f, 1.5f};
	const float sph_from[3][3] = {{0.3f, -0.2f, 1.5f}, {-0.7f, 0.1f, 0.45f}, {2.f, 3.f, -1.f}};
	const char *sph_name[3] = {"sphere_0_05", "sphere_0_4", "sphere_1_5"};
	for(int k = 0; k < 3; ++k)
	{
		Params p; p.str("type", "spherelight"); p.p("from", sph_from[k][0], sph_from[k][1], sph_from[k][2]); p.f("radius", sph_radius[k]);
		p.c("color", 0.7f, 0.8f, 0.9f - 0.2f * k); p.f("power", 5.f * (k + 1)); p.i("samples", 1 + 2 * k);
		add(sph_name[k]); sphere(j, sph_name[k], p, Point3(sph_from[k][0], sph_from[k][1], sph_from[k][2]), sph_radius[k]);
	}
	j.raw("sets", "[" + names + "]");
	printf("{\n%s\n}\n", j.s.c_str());
	return 0;
}
