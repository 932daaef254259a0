// TEST INFRASTRUCTURE — not product code.
//
// Reference harness for the spot light and the IES light.  Our driver, compiled (oracle/Makefile, target `ref`) against the reference's
// own headers and sources where they lie: light/light_spot.cc and light/light_ies.cc (with utility/util_ies.h) on top of the component
// objects.  Nothing of the reference is copied.
//
// Every light is made by the reference's factory() from a ParamMap, and the map is stored in the document, so the factory conversions
// (degrees to the two cosines through double and back, icos_diff_, colour times power, the cone of an IES file) are pinned with the leaf
// functions:
//
//   SpotLight::illuminate    in3 = p              out8 = ok, wi.dir_, wi.tmax_, colour
//   SpotLight::illumSample   in5 = p, s_1, s_2    out9 = ok, wi.dir_, wi.tmax_, s.pdf_, s.col_
//   SpotLight::intersect     in6 = from, dir      out6 = ok, t, ipdf, colour
//   IesLight::illuminate, ::illumSample           as the spot light's, with a mark per row (below)
//   IesData::getRadiance     in2 = h_ang, v_ang   out1 = radiance          (degrees; an IesData of the driver's own, parseIesFile first)
//   diracLight(), canIntersect(), nSamples() of each light  flags3
//
// (the outputs of a refused call are zeros).  The spot lights are the eight of LEAF in tests/test_gpu_spot.py and its eight intersect
// lights at the world origin and at (0.05, 0, 0); the IES lights read the seven files of tests/ies_fixture.py, which
// tests/golden/make_golden.py writes into a directory and names on the command line, each once as a Dirac light and once with soft_shadows.
// The document stores the file's name only.
//
// THE MARK.  At or beyond the last entry of an angle map the scans of IesData::getRadiance read one element past their arrays: what
// the reference answers there is undefined and no fixture value.  The driver decides from the parsed maps (the fold by photometric type,
// then the comparison with each map's last entry) whether a lookup lands there and writes a 1 into the row's mark; tests skip marked
// rows.  Rows that are drawn freely (the plane across the axis, the box) are drawn again while they are marked, and at most 5 % of a
// leaf's rows may be marked.  For the type B file this keeps the directions with a negative world y out: its vertical map ends at 90 and
// the horizontal angle of such a direction, 180 to 360, folds to 90 or more; the axis itself (vertical angle 0, which type B turns into
// exactly 90) is past its map too, which is why an IES light gets few rows there, and few on its cone's rim, where the vertical angle is the
// map's last entry.
//
// THE CONE ROWS.  A row "on" cos_end_ or cos_start_ or a float neighbour of either is drawn until the cosine to the axis that the REFERENCE
// forms there is exactly that float: the driver puts the float and the one above it into the light's cos_end_ and asks its own cone test
// (cosine_is below; cos_end_ is put back before anything is recorded).  So each build's rows sit at its own thresholds, and where the
// two builds form a threshold a float step apart (the 5 degree cone) those rows differ between the two fixtures; all other rows are the
// same in both, each row drawing from a stream of its own.
//
// The conditions on the inputs are asserted here while generating; see require() below.  The edge rows come first in every leaf, the
// seeded ones after them.
//
// Output: one JSON document on stdout, floats as IEEE-754 bit patterns.  tests/golden/make_golden.py stores it as
// tests/golden/ref_spot_ies_{ieee,fast}.json.gz.

// the standard library first: its headers must not see the macro below
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#define private public
#include "common/param.h"
#include "common/surface.h"
#include "common/scene.h"
#include "common/ray.h"
#include "light/light_spot.h"
#include "light/light_ies.h"
#include "utility/util_ies.h"
#undef private

using namespace yafaray4;

static const int N_SPOT = 600, N_INT = 520, N_IES = 400, N_LOOKUP = 1000;
static const int G = 48;          // rows per group of special points
static const int GA = 8;          // rows on the axis before the light, and behind it
static const int GC_IES = 6;      // rows per cosine on an IES light's cone: its rim is the end of the vertical map, where most lookups are past it

// The inputs are formed in plain IEEE arithmetic on bare components in both builds of this driver (none of the reference's inline
// operators, which the release-flag build compiles its own way), so that the two fixtures ask the reference the same questions row by row
#pragma GCC push_options
#pragma GCC optimize("no-fast-math")
static uint32_t lcg_state = 41011u;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }
// every row draws from a stream of its own (light, leaf, row): a row that is drawn again, a different number of times in the two builds,
// leaves the rows after it alone
static int light_index = 0;
static void seed_row(int leaf, int k) { lcg_state = 41011u + 2654435761u * (uint32_t)(light_index * 4 + leaf) + 40503u * (uint32_t)k; lcg(); lcg(); }
static float urand() { return (float)((lcg() >> 8) * (1.0 / 16777216.0)); }
static float srand11() { return 2.f * urand() - 1.f; }
static float uniform(float a, float b) { return a + (b - a) * urand(); }
static uint32_t f2u(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
static const float ONE_BELOW = 0.99999994f;       // the float below 1

static Vec3 unit(float x, float y, float z)
{
	const float inv = 1.f / std::sqrt(x * x + y * y + z * z);
	return Vec3(x * inv, y * inv, z * inv);
}

static Vec3 rand_unit()
{
	for(;;)
	{
		const float x = srand11(), y = srand11(), z = srand11(), l = x * x + y * y + z * z;
		if(l > 0.01f && l < 1.f) return unit(x, y, z);
	}
}
#pragma GCC pop_options

static void require(bool ok, const char *what, const std::string &set, double value)
{
	if(ok) return;
	fprintf(stderr, "ref_spot_ies: %s: %s (%g)\n", set.c_str(), what, value);
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
	// (the factory reads the file where make_golden.py wrote it; the document keeps its name)
	void file(const std::string &dir, const std::string &name) { pm["file"] = Parameter(dir + "/" + name); sep(); json += "\"file\": \"" + name + "\""; }
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

// ---- the points around a light (plain IEEE arithmetic again) --------------------------------------------------------
#pragma GCC push_options
#pragma GCC optimize("no-fast-math")
// a light's frame as its constructor left it (read from the object: nothing is formed again here)
struct Frame { Point3 pos; Vec3 ndir, du, dv; };

static float radius(int k) { return (k % 2 == 0) ? uniform(0.2f, 1.f) : uniform(1.f, 3.f); }      // half nearer than 1: both branches of the spot's pdf patch

// a point whose direction TO the light makes the cosine cc with ndir_
static Point3 on_cone(const Frame &f, double cc, int k)
{
	cc = std::min(1.0, std::max(-1.0, cc));
	const double phi = 6.283185307179586 * urand(), s = std::sqrt(std::max(1.0 - cc * cc, 0.0)), r = radius(k);
	const double d[3] = {f.ndir.x_ * cc + (f.du.x_ * std::cos(phi) + f.dv.x_ * std::sin(phi)) * s,
	                     f.ndir.y_ * cc + (f.du.y_ * std::cos(phi) + f.dv.y_ * std::sin(phi)) * s,
	                     f.ndir.z_ * cc + (f.du.z_ * std::cos(phi) + f.dv.z_ * std::sin(phi)) * s};
	return Point3((float)(f.pos.x_ - r * d[0]), (float)(f.pos.y_ - r * d[1]), (float)(f.pos.z_ - r * d[2]));
}

// is the cosine to the axis that the REFERENCE forms at p exactly `target`?  (asked through the light's own cone test: cosine_is below)
typedef bool (*CosineIs)(const Light *, const Point3 &, float);

// row k of a leaf's points.  The kinds, in order: the light's own position; G on the plane through the light across its axis; G on each
// cone in `cones` and G on each of its cosine's float neighbours, drawn until the reference's own cosine there IS that float (400 draws
// at the most: a neighbour beyond +-1 cannot be met); G between the first two cones (the falloff band) where they differ; GA on
// the axis before the light and GA behind it; a box of +-3 around the light from there on.  special_rows: how many rows come before the box
static int special_rows(const std::vector<float> &cones, int gc) { return 1 + G + 3 * gc * (int)cones.size() + ((cones.size() > 1 && cones[0] != cones[1]) ? G : 0) + 2 * GA; }

static Point3 along(const Point3 &o, float a, const Vec3 &u, float b, const Vec3 &v)
{
	return Point3(o.x_ + a * u.x_ + b * v.x_, o.y_ + a * u.y_ + b * v.y_, o.z_ + a * u.z_ + b * v.z_);
}

static Point3 point_row(const Frame &f, const std::vector<float> &cones, int gc, int k, const Light *l, CosineIs cosine_is)
{
	if(k == 0) return f.pos;
	k -= 1;
	if(k < G) { const float a = uniform(-2.f, 2.f), b = uniform(-2.f, 2.f); return along(f.pos, a, f.du, b, f.dv); }
	k -= G;
	for(float c : cones)
	{
		const float cc[3] = {c, std::nextafter(c, 2.f), std::nextafter(c, -2.f)};
		if(k < 3 * gc)
		{
			Point3 p = on_cone(f, cc[k / gc], k);
			for(int t = 0; t < 400 && !cosine_is(l, p, cc[k / gc]); ++t) p = on_cone(f, cc[k / gc], k);
			return p;
		}
		k -= 3 * gc;
	}
	if(cones.size() > 1 && cones[0] != cones[1])
	{
		if(k < G) return on_cone(f, (double)cones[0] + ((double)cones[1] - (double)cones[0]) * urand(), k);
		k -= G;
	}
	if(k < GA) return along(f.pos, -radius(k), f.ndir, 0.f, f.ndir);        // on the axis, lit
	k -= GA;
	if(k < GA) return along(f.pos, radius(k), f.ndir, 0.f, f.ndir);         // behind the light
	const float x = 3.f * srand11(), y = 3.f * srand11(), z = 3.f * srand11();
	return Point3(f.pos.x_ + x, f.pos.y_ + y, f.pos.z_ + z);
}

// the rows that are not drawn again when their lookup is past the maps: the light's position, the cone rows, the axis
static bool fixed_row(const std::vector<float> &cones, int gc, int k) { return k == 0 || (k >= 1 + G && k < special_rows(cones, gc)); }

// the eight sample pairs with 0 and the float below 1, on the first rows of the axis before the light (accepted); seeded otherwise
static void sample_row(const std::vector<float> &cones, int gc, int k, float &s_1, float &s_2)
{
	static const float e[8][2] = {{0.f, 0.f}, {0.f, ONE_BELOW}, {ONE_BELOW, 0.f}, {ONE_BELOW, ONE_BELOW}, {0.f, 0.5f}, {0.5f, 0.f}, {ONE_BELOW, 0.5f}, {0.5f, ONE_BELOW}};
	const int first = special_rows(cones, gc) - 2 * GA;
	s_1 = urand(); s_2 = urand();
	if(k >= first && k < first + 8) { s_1 = e[k - first][0]; s_2 = e[k - first][1]; }
}

#pragma GCC pop_options

// the light's cone test `cosa < cos_end_` answers for any threshold put into cos_end_: the cosine is `target` when it passes at `target`
// and fails at the float above.  cos_end_ is put back before anything is recorded
template<class L> static bool cosine_is(const Light *light, const Point3 &p, float target)
{
	L *l = const_cast<L *>(static_cast<const L *>(light));
	const float keep = l->cos_end_;
	SurfacePoint sp; surface_at(sp, p);
	Ray wi; Rgb col(0.f);
	l->cos_end_ = target;
	const bool at_least = l->illuminate(sp, col, wi);
	l->cos_end_ = std::nextafter(target, 2.f);
	const bool above = l->illuminate(sp, col, wi);
	l->cos_end_ = keep;
	return at_least && !above;
}

// ---- the spot light -------------------------------------------------------------------------------------------------
static void spot_leaves(Doc &j, const std::string &name, Params &pr, float blend)
{
	Light *l = SpotLight::factory(pr.pm, fake_env());
	const SpotLight *sl = static_cast<const SpotLight *>(l);
	++light_index;
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	const Frame f = {sl->position_, sl->ndir_, sl->du_, sl->dv_};
	const std::vector<float> cones = {sl->cos_end_, sl->cos_start_};
	require(special_rows(cones, G) < N_SPOT, "room for seeded rows", name, special_rows(cones, G));
	std::vector<uint32_t> in, out, sin, sout;
	int accepted = 0, near = 0, far = 0, band = 0, s_near = 0, s_far = 0;
	for(int k = 0; k < N_SPOT; ++k)
	{
		seed_row(0, k);
		const Point3 p = point_row(f, cones, G, k, l, cosine_is<SpotLight>);
		SurfacePoint sp; surface_at(sp, p);
		{
			Ray wi; Rgb col(0.f);
			bool ok = l->illuminate(sp, col, wi);
			if(ok)
			{
				++accepted; near += wi.tmax_ < 1.f; far += wi.tmax_ > 1.f;
				band += (sl->ndir_ * wi.dir_) < sl->cos_start_;
			}
			else { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; col = Rgb(0.f); }
			pushp(in, p);
			out.push_back(f2u(ok ? 1.f : 0.f)); pushv(out, wi.dir_); out.push_back(f2u(wi.tmax_)); pushc(out, col);
		}
		{
			LSample ls; sample_row(cones, G, k, ls.s_1_, ls.s_2_); ls.pdf_ = 0.f; ls.col_ = Rgb(0.f);
			Ray wi; wi.from_ = p;
			bool ok = l->illumSample(sp, ls, wi);
			if(ok) { s_near += ls.pdf_ == 1.f && wi.tmax_ < 1.f; s_far += ls.pdf_ > 1.f; }
			else { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; ls.pdf_ = 0.f; ls.col_ = Rgb(0.f); }
			pushp(sin, p); sin.push_back(f2u(ls.s_1_)); sin.push_back(f2u(ls.s_2_));
			sout.push_back(f2u(ok ? 1.f : 0.f)); pushv(sout, wi.dir_); sout.push_back(f2u(wi.tmax_)); sout.push_back(f2u(ls.pdf_)); pushc(sout, ls.col_);
		}
	}
	require(accepted * 10 >= N_SPOT && accepted * 10 <= N_SPOT * 9, "a spot light must accept 10 % to 90 % of the points", name, accepted);
	require(near >= 50 && far >= 50 && s_near >= 50 && s_far >= 50, "accepted points nearer than 1 and farther than 1 (both colour branches of illumSample)", name, std::min(std::min(near, far), std::min(s_near, s_far)));
	if(blend > 0.f) require(band >= 100, "at least 100 accepted points in the falloff band", name, band);
	else require(band == 0, "blend 0 has no falloff band", name, band);
	j.arr_u32(name + "_illuminate_in3", in); j.arr_u32(name + "_illuminate_out8", out);
	j.arr_u32(name + "_illum_sample_in5", sin); j.arr_u32(name + "_illum_sample_out9", sout);
}

// rays at a light at or near the world origin: from origins on a grid of dyadic offsets aimed through the light, which can meet the
// exact-zero test of intersect(), then seeded rays, which meet it by luck alone -> the number of rays answered true
static int spot_intersect(Doc &j, const std::string &name, Params &pr)
{
	Light *l = SpotLight::factory(pr.pm, fake_env());
	const SpotLight *sl = static_cast<const SpotLight *>(l);
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	static const float g[7] = {-2.f, -1.f, -0.5f, 0.f, 0.5f, 1.f, 2.f};
	++light_index; seed_row(2, 0);
	std::vector<uint32_t> in, out;
	int n = 0, answered = 0;
	auto one = [&](const Point3 &from, const Vec3 &d)
	{
		Ray ray(from, d);
		float t = 0.f, ipdf = 0.f; Rgb col(0.f);
		bool ok = l->intersect(ray, t, col, ipdf);
		if(!ok) { t = 0.f; ipdf = 0.f; col = Rgb(0.f); }
		answered += ok; ++n;
		pushp(in, from); pushv(in, d);
		out.push_back(f2u(ok ? 1.f : 0.f)); out.push_back(f2u(t)); out.push_back(f2u(ipdf)); pushc(out, col);
	};
	for(int a = 0; a < 7; ++a) for(int b = 0; b < 7; ++b) for(int c = 0; c < 7; ++c)
	{
		if(g[a] == 0.f && g[b] == 0.f && g[c] == 0.f) continue;
		const Point3 from(sl->position_.x_ + g[a], sl->position_.y_ + g[b], sl->position_.z_ + g[c]);
		one(from, unit(-g[a], -g[b], -g[c]));
	}
	while(n < N_INT) { const float x = 2.f * srand11(), y = 2.f * srand11(), z = 2.f * srand11(); one(Point3(x, y, z), rand_unit()); }
	j.arr_u32(name + "_intersect_in6", in); j.arr_u32(name + "_intersect_out6", out);
	return answered;
}

// ---- the IES light --------------------------------------------------------------------------------------------------
// does getRadiance(h_ang, v_ang) scan at or beyond the last entry of a map?  The fold by photometric type as the lookup applies it, then
// the comparison with the parsed maps' last entries
static bool past_the_maps(const IesData &d, float h_ang, float v_ang)
{
	float ang_1 = h_ang, ang_2 = v_ang;
	if(d.type_ != IesData::TypeC)
	{
		ang_1 = v_ang; ang_2 = h_ang;
		if(d.type_ == IesData::TypeB) { ang_1 += 90; if(ang_1 > 360.f) ang_1 -= 360.f; }
	}
	const float h_last = d.hor_angle_map_[d.hor_angles_ - 1], v_last = d.vert_angle_map_[d.vert_angles_ - 1];
	if(ang_1 > 180.f && h_last <= 180.f) ang_1 = 360.f - ang_1;
	if(ang_1 > 90.f && h_last <= 90.f) ang_1 -= 90.f;
	if(ang_2 > 90.f && v_last <= 90.f) ang_2 -= 90.f;
	return !(ang_1 < h_last) || !(ang_2 < v_last);
}

static void ies_lookup(Doc &j, const std::string &name, const std::string &path)
{
	IesData d;
	require(d.parseIesFile(path), "the file must parse", name, 0);
	++light_index; seed_row(3, 0);
	std::vector<float> hor(d.hor_angle_map_, d.hor_angle_map_ + d.hor_angles_), vert(d.vert_angle_map_, d.vert_angle_map_ + d.vert_angles_);
	std::vector<uint32_t> in, out, mark;
	int n = 0, marked = 0;
	auto one = [&](float h, float v)
	{
		const bool m = past_the_maps(d, h, v);
		const float rad = m ? 0.f : d.getRadiance(h, v);
		in.push_back(f2u(h)); in.push_back(f2u(v)); out.push_back(f2u(rad)); mark.push_back(m);
		marked += m; ++n;
	};
	auto seeded = [&](float &h, float &v) { for(int t = 0; t < 200; ++t) { h = uniform(0.f, 360.f); v = uniform(0.f, 180.f); if(!past_the_maps(d, h, v)) return; } };
	// every node of one map with every node of the other, in both orders (which angle meets which map depends on the photometric type):
	// the exact-hit branch
	for(float a : hor) for(float b : vert) { one(a, b); one(b, a); }
	// every node, both ends among them, and 90 / 180 / 360, each with its float neighbours, as either angle beside a seeded one
	std::vector<float> nodes(hor); nodes.insert(nodes.end(), vert.begin(), vert.end());
	nodes.push_back(90.f); nodes.push_back(180.f); nodes.push_back(360.f);
	std::sort(nodes.begin(), nodes.end()); nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
	for(float a : nodes)
	{
		const float beside[3] = {a, std::nextafter(a, 1e9f), std::nextafter(a, -1e9f)};
		for(float b : beside)
		{
			float h, v;
			// the seeded partner is drawn until the pair is inside the maps, where the node's own angle leaves that open
			for(int t = 0; t < 200; ++t) { seeded(h, v); if(!past_the_maps(d, b, v)) break; }
			one(b, v);
			for(int t = 0; t < 200; ++t) { seeded(h, v); if(!past_the_maps(d, h, b)) break; }
			one(h, b);
		}
	}
	require(n < N_LOOKUP, "room for seeded pairs", name, n);
	while(n < N_LOOKUP) { float h, v; seeded(h, v); one(h, v); }
	fprintf(stderr, "ref_spot_ies: %s: %d of %d lookups past the maps\n", name.c_str(), marked, n);
	require(marked * 20 <= n, "at most 5 % of the lookups past the maps", name, marked);
	j.arr_u32(name + "_radiance_in2", in); j.arr_u32(name + "_radiance_out1", out); j.arr_u32(name + "_radiance_mark", mark);
}

static void ies_leaves(Doc &j, const std::string &name, Params &pr)
{
	Light *l = IesLight::factory(pr.pm, fake_env());
	require(l != nullptr, "the factory must accept the file", name, 0);
	const IesLight *il = static_cast<const IesLight *>(l);
	const IesData &d = *il->ies_data_;
	++light_index;
	j.raw(name + "_params", "{" + pr.json + "}");
	flags(j, name, l);
	const Frame f = {il->position_, il->ndir_, il->du_, il->dv_};
	const std::vector<float> cones = {il->cos_end_};
	require(special_rows(cones, GC_IES) < N_IES, "room for seeded rows", name, special_rows(cones, GC_IES));
	std::vector<uint32_t> in, out, mark, sin, sout, smark;
	int accepted = 0, marked = 0, s_accepted = 0, s_marked = 0;
	// the lookup of a call at p: illuminate's own direction to the light gives the cosine both functions hand to getAngles
	auto lookup_past = [&](const Point3 &p, const Vec3 *sampled) -> bool
	{
		SurfacePoint sp; surface_at(sp, p);
		Ray wi; Rgb col(0.f);
		if(!l->illuminate(sp, col, wi)) return false;          // refused before any lookup
		const float cosa = il->ndir_ * wi.dir_;
		float u, v;
		il->getAngles(u, v, sampled ? *sampled : wi.dir_, cosa);
		return past_the_maps(d, u, v);
	};
	for(int k = 0; k < N_IES; ++k)
	{
		{
			seed_row(0, k);
			Point3 p = point_row(f, cones, GC_IES, k, l, cosine_is<IesLight>);
			for(int t = 0; t < 200 && !fixed_row(cones, GC_IES, k) && lookup_past(p, nullptr); ++t) p = point_row(f, cones, GC_IES, k, l, cosine_is<IesLight>);
			const bool m = lookup_past(p, nullptr);
			SurfacePoint sp; surface_at(sp, p);
			Ray wi; Rgb col(0.f);
			bool ok = !m && l->illuminate(sp, col, wi);
			if(!ok) { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; col = Rgb(0.f); }
			accepted += ok; marked += m;
			pushp(in, p); mark.push_back(m);
			out.push_back(f2u(ok ? 1.f : 0.f)); pushv(out, wi.dir_); out.push_back(f2u(wi.tmax_)); pushc(out, col);
		}
		{
			Point3 p; LSample ls; Ray wi; bool ok = false, m = false;
			seed_row(1, k);
			for(int t = 0; t < 200; ++t)
			{
				p = point_row(f, cones, GC_IES, k, l, cosine_is<IesLight>);
				sample_row(cones, GC_IES, k, ls.s_1_, ls.s_2_); ls.pdf_ = 0.f; ls.col_ = Rgb(0.f);
				SurfacePoint sp; surface_at(sp, p);
				wi = Ray(); wi.from_ = p;
				// (the sampled direction is written before the lookup, whatever the lookup then answers)
				wi.dir_ = Vec3(0.f);
				ok = l->illumSample(sp, ls, wi);
				m = lookup_past(p, &wi.dir_);
				if(!m || fixed_row(cones, GC_IES, k)) break;
			}
			if(m) ok = false;
			if(!ok) { wi.dir_ = Vec3(0.f); wi.tmax_ = 0.f; ls.pdf_ = 0.f; ls.col_ = Rgb(0.f); }
			s_accepted += ok; s_marked += m;
			pushp(sin, p); sin.push_back(f2u(ls.s_1_)); sin.push_back(f2u(ls.s_2_)); smark.push_back(m);
			sout.push_back(f2u(ok ? 1.f : 0.f)); pushv(sout, wi.dir_); sout.push_back(f2u(wi.tmax_)); sout.push_back(f2u(ls.pdf_)); pushc(sout, ls.col_);
		}
	}
	require(accepted * 10 >= N_IES && s_accepted * 10 >= N_IES, "an IES light must accept 10 % of the points", name, std::min(accepted, s_accepted));
	fprintf(stderr, "ref_spot_ies: %s: accepted %d / %d, past the maps %d / %d of %d\n", name.c_str(), accepted, s_accepted, marked, s_marked, N_IES);
	require(marked * 20 <= N_IES && s_marked * 20 <= N_IES, "at most 5 % of a leaf's rows past the maps", name, std::max(marked, s_marked));
	j.arr_u32(name + "_illuminate_in3", in); j.arr_u32(name + "_illuminate_out8", out); j.arr_u32(name + "_illuminate_mark", mark);
	j.arr_u32(name + "_illum_sample_in5", sin); j.arr_u32(name + "_illum_sample_out9", sout); j.arr_u32(name + "_illum_sample_mark", smark);
}

int main(int argc, char **argv)
{
	if(argc != 2) { fprintf(stderr, "usage: ref_spot_ies <directory with the IES files of tests/ies_fixture.py>\n"); return 2; }
	const std::string dir = argv[1];
	Doc j;
	std::string spots, intersects, ies, files;
	auto add = [](std::string &names, const std::string &n) { if(!names.empty()) names += ", "; names += "\"" + n + "\""; };

	// cone_angle, blend, shadowFuzzyness, soft_shadows: blends 0 / 0.15 / 1, cone angles 5 / 45 / 120, fuzzyness 0 / 0.5 / 1, both kinds
	static const float leaf[8][3] = {{45.f, 0.15f, 1.f}, {45.f, 0.f, 1.f}, {45.f, 1.f, 0.5f}, {5.f, 0.15f, 1.f}, {5.f, 1.f, 0.f}, {120.f, 0.15f, 0.5f}, {120.f, 0.f, 0.f}, {120.f, 1.f, 1.f}};
	static const bool leaf_soft[8] = {false, false, true, true, false, true, true, false};
	for(int k = 0; k < 8; ++k)
	{
		Params p; p.str("type", "spotlight"); p.p("from", 0.25f, -0.5f, 2.f); p.p("to", 0.75f, 0.25f, 0.f); p.c("color", 0.9f, 0.7f, 0.3f); p.f("power", 5.f);
		p.f("cone_angle", leaf[k][0]); p.f("blend", leaf[k][1]); p.f("shadowFuzzyness", leaf[k][2]); p.b("soft_shadows", leaf_soft[k]); p.i("samples", 2);
		const std::string name = "spot" + std::to_string(k);
		add(spots, name); spot_leaves(j, name, p, leaf[k][1]);
	}
	// intersect(): lights at the world origin and at (0.05, 0, 0), axes along -+z and -+x
	static const float at[2] = {0.f, 0.05f};
	static const float axis[4][3] = {{0.f, 0.f, -1.f}, {0.f, 0.f, 1.f}, {-1.f, 0.f, 0.f}, {1.f, 0.f, 0.f}};
	// [at the origin, at x = 0.05 with the axis along z, at x = 0.05 with the axis along x]
	int answered[3] = {0, 0, 0};
	for(int k = 0; k < 8; ++k)
	{
		const float x = at[k / 4], *a = axis[k % 4];
		// (`to` as tests/test_gpu_spot.py writes it: from + axis where the axis is along z, the axis itself where it is along x)
		Params p; p.str("type", "spotlight"); p.p("from", x, 0.f, 0.f); p.p("to", (k % 4 < 2) ? x + a[0] : a[0], a[1], a[2]); p.c("color", 0.9f, 0.7f, 0.3f); p.f("power", 5.f);
		p.f("cone_angle", 45.f); p.f("blend", 0.5f); p.b("soft_shadows", true); p.i("samples", 2);
		const std::string name = "int" + std::to_string(k);
		add(intersects, name); answered[k < 4 ? 0 : (k < 6 ? 1 : 2)] += spot_intersect(j, name, p);
	}
	// At the origin the products of the plane test round back to zero for many rays.  At x = 0.05 with the axis along z the light's plane is
	// still z = 0 and the hit point (0.05, 0, 0) lies within 0.1 of the world origin: the reference answers true there too.  With the axis
	// along x the offset along the axis is p.x - 0.05f, and 0.05f has more low bits than a sum of magnitude 0.5 to 2 keeps: never exactly zero
	require(answered[0] >= 50, "intersect() must answer true for at least 50 rays over the lights at the origin", "int0-3", answered[0]);
	require(answered[1] >= 10, "intersect() answers true at x = 0.05 where the axis is along z", "int4-5", answered[1]);
	require(answered[2] == 0, "intersect() must answer true for no ray at x = 0.05 with the axis along x", "int6-7", answered[2]);
	fprintf(stderr, "ref_spot_ies: intersect() answered true %d / %d / %d times\n", answered[0], answered[1], answered[2]);

	static const char *names[7] = {"B", "C1", "C5x7", "C90", "Cup", "FLAT", "TILT"};
	for(int k = 0; k < 7; ++k)
	{
		const std::string file = std::string(names[k]) + ".ies";
		add(files, names[k]); ies_lookup(j, std::string("file_") + names[k], dir + "/" + file);
		for(int soft = 0; soft <= 1; ++soft)
		{
			// (the axis leans to +y: the type B file's lookups along it stay inside its maps)
			Params p; p.str("type", "ieslight"); p.file(dir, file); p.p("from", 0.25f, -0.5f, 2.f); p.p("to", 0.75f, -1.25f, 0.f); p.c("color", 0.9f, 0.7f, 0.3f); p.f("power", 5.f);
			p.b("soft_shadows", soft); p.i("samples", 2 + k);
			const std::string name = std::string("ies_") + names[k] + (soft ? "_soft" : "_dirac");
			add(ies, name); ies_leaves(j, name, p);
		}
	}
	j.raw("spot_sets", "[" + spots + "]"); j.raw("intersect_sets", "[" + intersects + "]"); j.raw("ies_sets", "[" + ies + "]"); j.raw("ies_files", "[" + files + "]");
	std::cout.flush(); fflush(stdout);
	printf("{\n%s\n}\n", j.s.c_str());
	return 0;
}
