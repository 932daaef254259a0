// MI355X (gfx950) path-tracing core: flattened kd-tree traversal, surface shading with MIS direct
// lighting, and deterministic film accumulation — hand-written HIP.
//
// Reference path: TiledIntegrator::renderTile (integrator_tiled.cc:309-521) ->
// PathIntegrator::integrate (integrator_path_tracer.cc:112-347) -> Scene::intersect / isShadowed
// (scene.cc:896-994) -> TriKdTree::intersect / intersectS (kdtree_triangle.cc:684-977) ->
// Triangle::intersect (triangle.h:223-259), MonteCarloIntegrator::doLightEstimation
// (integrator_montecarlo.cc:78-345), ImageFilm::addSample (imagefilm.cc:925-1015).
//
// This unit holds the device scene, the pieces of traversal and shading the kernels share, the host side
// of the narrow ABI, and (through yafgpu_wavefront.h) the wavefront pass: a path runs as a coroutine that
// parks its state in HBM at every kd-tree query, and traversal kernels answer the queries in queues
// (DESIGN.md §4.1 has the full picture).  Traversal keeps a short per-lane stack in LDS ([slot][lane],
// conflict-free), with the classic kd-restart fallback when more than kStack far-children are pending.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <mutex>

#include "../../include/yafgpu.h"
#include "kdtree_build.h"
#include "yafgpu_math.h"
#include "yafgpu_shading.h"
#include "yafgpu_texture.h"
#include "yafgpu_assemble.h"

namespace yafgpu {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
#ifndef YAFGPU_STACK
#define YAFGPU_STACK 8                // 8 slots: 8 waves/SIMD for the traversal kernels, 0.8 % of rays restart (C2)
#endif
constexpr int kStack = YAFGPU_STACK;  // per-lane LDS stack slots (power of two): wf_trace holds kStack - 1 live entries (its node step writes the slot
                                      // above the top unconditionally), kd_trace_ts holds kStack; an older far child is overwritten and recovered by a kd-restart
constexpr int kDepthCap = 48;         // host tree depth cap; deeper pending lists restart
constexpr float kMinRayDist = (float)0.00005;   // MIN_RAYDIST, CMakeLists.txt:46-48
constexpr float kShadowBias = (float)0.0005;    // YAF_SHADOW_BIAS, CMakeLists.txt:50-52

// ------------------------------------------------------------------------------------------------
// device scene
struct DevScene
{
	const uint2 *nodes;          // 8-byte kd nodes (kdtree_build.h)
	const uint4 *treelets;       // the treelet layout of the same tree (kdtree_build.h, TreeletLayout): 2 x uint4 per treelet, walked by wf_trace
	const uint2 *tl_leaves;      // (first reference, count) of the leaves whose links escape (kLinkEscape)
	uint32_t tl_root;            // the link every walk of wf_trace starts at
	const uint32_t *refs;        // leaf references
	const float4 *tri;           // 3 x float4 per triangle: (a, eps) (e1, mat|vis<<30) (e2, 0)
	const float4 *tri_walk;      // wf_trace's own copy of the records, triangle t at position pos[t] (kdtree_build.h, tri_order: leaf order, or the
	                             // identity with YAFGPU_TRI_ORDER=id), the spare word of its third float4 holding t as bits; everything that takes a
	                             // hit's triangle id reads the arrays addressed by id
	const uint32_t *refs_walk;   // refs_walk[i] = pos[refs[i]]: the leaf references as positions in tri_walk
	const float4 *tri_ng;        // geometric normal + smooth flag
	const float4 *tri_vn;        // 3 x float4 per triangle (vertex normals) or nullptr
	const yafgpu_material *mats;
	const yafgpu_light *lights;
	const int *faure;            // concatenated Faure permutations — or a copy of their first faure_near ints (wf_shade stages a prefix in LDS)
	const int *faure_far;        // the whole table (global memory), for a dimension that reaches beyond faure_near
	const int *faure_off;        // [50] offsets into faure
	const double *inv_prims;     // [50]
	int n_lights, n_tris, n_mats, n_faure;      // n_faure: ints in the concatenated Faure permutations
	int faure_near;              // ints `faure` holds (n_faure unless a kernel staged a prefix)
	uint32_t n_nodes;
	float blo[3], bhi[3];
	yafgpu_camera cam;
	TexScene tex;                // textures, texels, shader nodes, per-triangle texture coordinates (nodes == nullptr: none)
	BgScene bg;                  // the background record and the background light's tables (kind 0: none; tab == nullptr: no light)
	const float *lgeo;           // the light-geometry pool of the mesh lights and the portals (nullptr: none): 9 floats per triangle (a, b, c) from
	                             // 9 * mesh_pool on, behind the triangles every light's Pdf1D row from mesh_row on (integral_, inv_integral_, func_,
	                             // cdf_), and behind the rows every portal's triangle records and normals from mesh_first on
};

struct RenderArgs
{
	DevScene sc;
	yafgpu_render_params rp;
	float shadow_bias, ray_min_dist, filterw;
	float table_scale; int wide_filter;   // wide_filter: footprint beyond the 2x2 box case -> table weights + atomics (wavefront accumulate)
	const float *filter_table;            // 16x16 reconstruction-filter table (ImageFilm ctor, imagefilm.cc:152-176)
	int n_tiles;
	const int4 *tile_rect;         // x0,y0,w,h per tile of this shard
	float *planes;
	yafgpu_counters *counters;
};

struct LaneCounters { uint32_t closest, shadow, interior, leaves, tests, samples, restarts; };

__constant__ int c_prims[50] = {1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67,
                                71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167,
                                173, 179, 181, 191, 193, 197, 199, 211, 223, 227};

// scrHalton__, include/common/scr_halton.h:52-75
YG_DEV double scr_halton(const DevScene &sc, int dim, uint32_t n)
{
	double value = 0.0;
	const uint32_t base = (uint32_t)c_prims[dim];
	const int off = sc.faure_off[dim];
	const int *sigma = (off + (int)base <= sc.faure_near ? sc.faure : sc.faure_far) + off;
	double f, factor, dn = (double)n;
	f = factor = sc.inv_prims[dim];
	while(n > 0)
	{
		value += (double)(sigma[n % base]) * factor;
		dn *= f;
		n = (uint32_t)dn;
		factor *= f;
	}
	return fmax(1.0e-36, fmin(1.0, value));
}

// Bound::cross, include/common/bound.h:144-212
// (inv_dir = 1/dir per component, computed once by the caller: the traversal needs the same three quotients)
YG_DEV bool bound_cross(const DevScene &sc, V3 from, V3 dir, V3 inv_dir, float dist, float &enter, float &leave)
{
	const V3 a0 = mk(sc.blo[0], sc.blo[1], sc.blo[2]), a1 = mk(sc.bhi[0], sc.bhi[1], sc.bhi[2]);
	const V3 p = from - a0;
	float lmin = -1e38f, lmax = 1e38f, ltmin, ltmax;
	if(dir.x != 0.f)
	{
		const float inv = inv_dir.x;
		if(inv > 0.f) { lmin = -p.x * inv; lmax = ((a1.x - a0.x) - p.x) * inv; }
		else { lmin = ((a1.x - a0.x) - p.x) * inv; lmax = -p.x * inv; }
		if((lmax < 0.f) || (lmin > dist)) return false;
	}
	if(dir.y != 0.f)
	{
		const float inv = inv_dir.y;
		if(inv > 0.f) { ltmin = -p.y * inv; ltmax = ((a1.y - a0.y) - p.y) * inv; }
		else { ltmin = ((a1.y - a0.y) - p.y) * inv; ltmax = -p.y * inv; }
		lmin = smax(ltmin, lmin);
		lmax = smin(ltmax, lmax);
		if((lmax < 0.f) || (lmin > dist)) return false;
	}
	if(dir.z != 0.f)
	{
		const float inv = inv_dir.z;
		if(inv > 0.f) { ltmin = -p.z * inv; ltmax = ((a1.z - a0.z) - p.z) * inv; }
		else { ltmin = ((a1.z - a0.z) - p.z) * inv; ltmax = -p.z * inv; }
		lmin = smax(ltmin, lmin);
		lmax = smin(ltmax, lmax);
		if((lmax < 0.f) || (lmin > dist)) return false;
	}
	if((lmin <= lmax) && (lmax >= 0.f) && (lmin <= dist)) { enter = lmin; leave = lmax; return true; }
	return false;
}

// Triangle::intersect, include/common/triangle.h:223-259, on the 48-byte record
YG_DEV bool tri_test(const float4 r0, const float4 r1, const float4 r2, V3 from, V3 dir, float &t, float &u, float &v)
{
	const V3 a = mk(r0.x, r0.y, r0.z), e1 = mk(r1.x, r1.y, r1.z), e2 = mk(r2.x, r2.y, r2.z);
	const float eps = r0.w;
	const V3 pvec = cross(dir, e2);
	const float det = dot(e1, pvec);
	if(det > -eps && det < eps) return false;
	const float inv_det = 1.f / det;
	const V3 tvec = from - a;
	u = dot(tvec, pvec) * inv_det;
	if(u < 0.f || u > 1.f) return false;
	const V3 qvec = cross(tvec, e1);
	v = dot(dir, qvec) * inv_det;
	if((v < 0.f) || ((u + v) > 1.f)) return false;
	t = dot(e2, qvec) * inv_det;
	if(t < eps) return false;
	return true;
}

// the same test, straight-line: identical operations and roundings, the four rejections combined at the end
// (a rejected lane may compute with inf / NaN on the way; its result is discarded)
YG_DEV bool tri_test_flat(const float4 r0, const float4 r1, const float4 r2, V3 from, V3 dir, float &t, float &u, float &v)
{
	const V3 a = mk(r0.x, r0.y, r0.z), e1 = mk(r1.x, r1.y, r1.z), e2 = mk(r2.x, r2.y, r2.z);
	const float eps = r0.w;
	const V3 pvec = cross(dir, e2);
	const float det = dot(e1, pvec);
	const bool det_ok = !(det > -eps && det < eps);
	const float inv_det = 1.f / det;
	const V3 tvec = from - a;
	u = dot(tvec, pvec) * inv_det;
	const bool u_ok = !(u < 0.f || u > 1.f);
	const V3 qvec = cross(tvec, e1);
	v = dot(dir, qvec) * inv_det;
	const bool v_ok = !((v < 0.f) || ((u + v) > 1.f));
	t = dot(e2, qvec) * inv_det;
	return det_ok && u_ok && v_ok && !(t < eps);
}

// per-lane stack in LDS: column `lane` of a [kStack][64] array of (node, tmax)
struct LaneStack
{
	uint2 *col;     // &stack[0][lane]; slot s lives at col[s * kWave]
	int sp, lo;     // entries [lo, sp) are live (ring of kStack); lo > 0: older pending far-children were overwritten
	YG_DEV void reset() { sp = 0; lo = 0; }
	YG_DEV bool empty() const { return sp == lo; }
	YG_DEV bool lost() const { return lo > 0; }      // a restart will recover what was overwritten
	YG_DEV void push(uint32_t node, float tmax)
	{
		col[(sp & (kStack - 1)) * kWave] = make_uint2(node, __float_as_uint(tmax));
		++sp;
		lo = max(lo, sp - kStack);
	}
	YG_DEV void pop(uint32_t &node, float &tmax)
	{
		--sp;
		const uint2 e = col[(sp & (kStack - 1)) * kWave];
		node = e.x; tmax = __uint_as_float(e.y);
	}
};

// Where a kd-restart resumes.  Normally at the exit of the cell just left.  If that cell had zero length (tmax == tmin)
// the walk may not have advanced at all since the previous restart: a tree with more split planes crossed at one
// distance than the short stack has slots (a degenerate chain of identical planes) would then restart at the same
// distance for ever.  Stepping to the next representable distance guarantees progress; what it can skip is a hit at
// exactly that distance in a zero-length cell of such a tree.
YG_DEV float restart_from(float tmin, float tmax)
{
	return (tmax > tmin) ? tmax : tmax + fmaxf(fabsf(tmax) * 1.2e-7f, 1e-30f);
}

// Triangle::getSurface, src/common/triangle.cc:30-133 (no UV / orco)
YG_DEV void get_surface(const DevScene &sc, int ti, V3 hitp, float bu, float bv, SurfPt &sp)
{
	const float4 g = sc.tri_ng[ti];
	sp.ng = mk(g.x, g.y, g.z);
	if(sc.tri_vn != nullptr && __float_as_uint(g.w) != 0u)
	{
		const float u = 1.f - bu - bv, v = bu, w = bv;   // b_0, b_1, b_2 (triangle.h:252-254, triangle.cc:34)
		const float4 na = sc.tri_vn[3 * ti], nb = sc.tri_vn[3 * ti + 1], nc = sc.tri_vn[3 * ti + 2];
		sp.n = normalize(mk(na.x, na.y, na.z) * u + mk(nb.x, nb.y, nb.z) * v + mk(nc.x, nc.y, nc.z) * w);
	}
	else sp.n = sp.ng;
	sp.mat = (int)(__float_as_uint(sc.tri[3 * ti + 1].w) & 0x3FFFFFFFu);
	sp.p = hitp;
	create_cs(sp.n, sp.nu, sp.nv);
}

// Transparent shadows: TriKdTree::intersectTs, kdtree_triangle.cc:983-1162.  Every triangle with ray_tmin <= t < dist
// whose material casts shadows either blocks the ray (opaque), or — once per triangle, the reference's std::set
// `filtered` — multiplies its transparency into filt; more than max_depth transparent triangles block it too.  The
// product is taken in visiting order, as there (so its last bits depend on tree topology, there as here).
constexpr int kTsMaxDepth = 8;
// kBlend: the walk of a scene in which some triangle uses a blend material (BlendMaterial::getTransparency at a crossing: the blend's node and
// two resolved records); every other scene's walk is compiled without it and keeps the registers and scratch it had.
template<bool kBlend>
YG_DEV bool kd_trace_ts(const DevScene &sc, LaneStack &stk, uint32_t *seen /* [kTsMaxDepth + 1] */, V3 from, V3 dir, float ray_tmin, float dist,
                        int max_depth, Col &filt)
{
	filt = mkc(1.f, 1.f, 1.f);
	float a, b;
	if(sc.n_nodes == 0u) return false;
	const V3 inv_dir = mk(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
	if(!bound_cross(sc, from, dir, inv_dir, dist, a, b)) return false;
	const float t_exit = b;
	float tmin = smax(a, 0.f), tmax = t_exit;
	uint32_t node = 0u;
	int depth = 0, n_seen = 0;
	stk.reset();
	for(;;)
	{
		if(dist < tmin) break;
		uint2 nd = sc.nodes[node];
		while((nd.y & 3u) != 3u)
		{
			const int axis = (int)(nd.y & 3u);
			const float split = __uint_as_float(nd.x);
			const float o = comp(from, axis), d = comp(dir, axis);
			const float tplane = (split - o) * comp(inv_dir, axis);
			const bool below = (o < split) || (o == split && d <= 0.f);
			const uint32_t left = node + 1u, right = nd.y >> 2;
			const uint32_t near_c = below ? left : right, far_c = below ? right : left;
			if(!(tplane <= tmax) || tplane <= 0.f) node = near_c;
			else if(tplane < tmin) node = far_c;
			else { stk.push(far_c, tmax); node = near_c; tmax = tplane; }
			nd = sc.nodes[node];
		}
		const uint32_t np = nd.y >> 2, first = nd.x;
		for(uint32_t i = 0; i < np; ++i)
		{
			const uint32_t ti = sc.refs[first + i];
			const float4 r0 = sc.tri[3u * ti], r1 = sc.tri[3u * ti + 1u], r2 = sc.tri[3u * ti + 2u];
			float t, u, v;
			if(!tri_test(r0, r1, r2, from, dir, t, u, v)) continue;
			const uint32_t vis = __float_as_uint(r1.w) >> 30;
			if(!(t < dist && t >= ray_tmin && (vis == 0u || vis == 2u))) continue;
			const yafgpu_material *mp = &sc.mats[__float_as_uint(r1.w) & 0x3FFFFFFFu];
#if YAFGPU_FEAT_TEXTURE
			const bool masked = sc.tex.nodes != nullptr && mp->type == YAFGPU_MAT_MASKED;
			const bool blended = kBlend && mp->type == YAFGPU_MAT_BLEND;
			// MaskMaterial::isTransparent, material_mask.cc:86-89, BlendMaterial::isTransparent, material_blend.cc:332-335: either sub-material's
			if((masked || blended) ? !mp->is_transparent : !mat_is_transparent(*mp)) return true;
#else
			if(!mat_is_transparent(*mp)) return true;
#endif
			bool known = false;
			for(int k = 0; k < n_seen; ++k) known = known || (seen[k * kWave] == ti);
			if(known) continue;
			if(depth >= max_depth) return true;
			if(n_seen <= kTsMaxDepth) seen[(n_seen++) * kWave] = ti;
			SurfPt sp;
			get_surface(sc, (int)ti, from + dir * t, u, v, sp);
#if YAFGPU_FEAT_TEXTURE
			// MaskMaterial::getTransparency, :91-99: the mask's nodes again, against 0.5 and not threshold_; the chosen material's
			// getTransparency follows, black for one that is opaque (the ray goes on with nothing left to carry)
			if(masked) mp = &sc.mats[mask_select(sc.tex, sc.cam, *mp, (int)ti, u, v, sp.p, sp.n, sp.ng, true)];
			if(kBlend && blended)
			{	// BlendMaterial::getTransparency, material_blend.cc:337-361: both sub-materials' filters (black for an opaque one) mixed by the
				// blend value at the crossing.  intersectTs calls no initBsdf (kdtree_triangle.cc:1105-1116): the surface point is the triangle's own
				BlendScratch b;
				blend_at_hit(sc.tex, sc.cam, sc.mats, *mp, (int)ti, u, v, sp.p, sp.n, sp.ng, b);
				filt = filt * blend_transparency(b, sp, dir);
				++depth;
				continue;
			}
#endif
			const yafgpu_material &m = *mp;
			if(m.n_nodes > 0 && sc.tex.nodes != nullptr)
			{	// getTransparency reads the diffuse shader and the component nodes (material_shiny_diffuse.cc:541-563)
				TexPoint tp; tex_point(sc.tex, (int)ti, u, v, sp.p, sp.n, sp.ng, tp);
				yafgpu_material tmp; mat_resolve(sc.tex, sc.cam, m, tp, tmp);
				filt = filt * mat_transparency(tmp, sp, dir);
			}
			else filt = filt * mat_transparency(m, sp, dir);
			++depth;
		}
		if(stk.empty())
		{
			if(!stk.lost() || tmax >= t_exit) break;
			tmin = restart_from(tmin, tmax); tmax = t_exit; node = 0u; stk.reset();
			continue;
		}
		tmin = tmax;
		stk.pop(node, tmax);
	}
	return false;
}

// stage of PathIntegrator::integrate (integrator_path_tracer.cc:112-347) a path's closest-hit query belongs to:
// the camera ray, a path sample's first segment from the camera hit, a later segment
enum : int { kStPrimary = 0, kStFirst = 1, kStDepth = 2 };

YG_DEV int round2int(double v) { return (int)(v + (.5 - 1.4e-11)); } // util_math.h:34-43

YG_DEV uint32_t wave_sum(uint32_t v)
{
#pragma unroll
	for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
	return v;
}

} // namespace yafgpu
#include "yafgpu_wavefront.h"
#ifndef YAFGPU_VARIANT_TU      // everything below: kernels and host code of the main unit
namespace yafgpu {

// film[y][x] = own + right(x-1,y) + down(x,y-1) + diag(x-1,y-1): the neighbours' splats onto this pixel
__global__ __launch_bounds__(kBlock) void combine_kernel(const float *planes, float *film, int w, int h)
{
	const size_t n = (size_t)w * (size_t)h;
	const size_t stride = n * YAFGPU_FILM_CHANNELS;
	for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
	{
		const int x = (int)(i % (size_t)w), y = (int)(i / (size_t)w);
#pragma unroll
		for(int c = 0; c < YAFGPU_FILM_CHANNELS; ++c)
		{
			float v = planes[i * YAFGPU_FILM_CHANNELS + c];
			if(x > 0) v += planes[stride + (i - 1) * YAFGPU_FILM_CHANNELS + c];
			if(y > 0) v += planes[2 * stride + (i - (size_t)w) * YAFGPU_FILM_CHANNELS + c];
			if(x > 0 && y > 0) v += planes[3 * stride + (i - (size_t)w - 1) * YAFGPU_FILM_CHANNELS + c];
			film[i * YAFGPU_FILM_CHANNELS + c] = v;
		}
	}
}

// Film files (ImageFilm::imageFilmLoadAllInFolder, imagefilm.cc:1520-1531): acc += film over the n = h * w * 5 floats of a film, col and
// weight alike, in float32; the first film is added to the zero film the reference starts from
__global__ __launch_bounds__(kBlock) void film_add_kernel(float *acc, const float *film, size_t n, int first)
{
	for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		acc[i] = (first ? 0.f : acc[i]) + film[i];
}

// The planes of a resumed render: the loaded film in the own plane, zero in the right, down and diagonal planes, so that combine_kernel
// gives the film back (x + 0 + 0 + 0) and the passes that follow add to it.  n = h * w * 5, the floats of one plane.
__global__ __launch_bounds__(kBlock) void seed_planes_kernel(const float *film, float *planes, size_t n)
{
	for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
	{
		planes[i] = film[i];
#pragma unroll
		for(int k = 1; k < YAFGPU_FILM_PLANES; ++k) planes[(size_t)k * n + i] = 0.f;
	}
}

// Component probe: evaluates the device-side restatements of the reference's leaf functions on
// arrays, so that tests can pin them against the reference's own golden vectors (tests/golden).
// Integers travel as float bit patterns.  One thread per item; no LDS, no traversal.
__global__ __launch_bounds__(kBlock) void probe_kernel(const DevScene sc, int op, int n, const float *in, int n_in, float *out, int n_out)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if(i >= n) return;
	const float *x = in + (size_t)i * (size_t)n_in;
	float *o = out + (size_t)i * (size_t)n_out;
	switch(op)
	{
		case 1:
		{
			const float ax = fabsf(x[0]) + 1e-3f;
			o[0] = f_sin(x[0]); o[1] = f_cos(x[0]); o[2] = f_exp2(x[0]); o[3] = f_log2(ax); o[4] = f_sqrt(ax);
			break;
		}
		case 2: o[0] = f_pow(x[0], x[1]); break;
		case 3:
		{
			const uint32_t bits = __float_as_uint(x[0]), r = __float_as_uint(x[1]);
			o[0] = ri_vdc(bits, r); o[1] = ri_lp(bits, r); o[2] = __uint_as_float(fnv32a(bits)); o[3] = ri_s(bits, r);
			break;
		}
		case 4:
		{
			const double v = scr_halton(sc, (int)__float_as_uint(x[0]), __float_as_uint(x[1]));
			o[0] = (float)v;
			o[1] = __uint_as_float((uint32_t)(__double_as_longlong(v) & 0xffffffffll));
			o[2] = __uint_as_float((uint32_t)((unsigned long long)__double_as_longlong(v) >> 32));
			break;
		}
		case 5:
		{
			Halton h; h.init(__float_as_uint(x[0])); h.set_start(__float_as_uint(x[1]));
			for(int k = 0; k < 6; ++k) o[k] = h.next();
			break;
		}
		case 6:
		{
			const V3 nn = mk(x[0], x[1], x[2]);
			V3 u, v; create_cs(nn, u, v);
			const V3 w = sample_cos_hemisphere(nn, u, v, x[3], x[4]);
			o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = v.x; o[4] = v.y; o[5] = v.z; o[6] = w.x; o[7] = w.y; o[8] = w.z;
			break;
		}
		case 7:
		{
			V3 f, d; float t0, t1, wt;
			if(n_in >= 4) camera_shoot<true>(sc.cam, x[0], x[1], x[2], x[3], f, d, t0, t1, wt);
			else camera_shoot<true>(sc.cam, x[0], x[1], 0.5f, 0.5f, f, d, t0, t1, wt);
			o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = t0; o[7] = t1; o[8] = wt;
			break;
		}
		case 8:
		{
			const yafgpu_light &l = sc.lights[0];
			V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f;
			const bool ok = arealight_illum_sample(l, mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf);
			o[0] = ok ? 1.f : 0.f;
			o[1] = ok ? d.x : 0.f; o[2] = ok ? d.y : 0.f; o[3] = ok ? d.z : 0.f; o[4] = ok ? tmax : 0.f; o[5] = ok ? pdf : 0.f;
			o[6] = ok ? l.color[0] : 0.f; o[7] = ok ? l.color[1] : 0.f; o[8] = ok ? l.color[2] : 0.f;
			break;
		}
		case 9:
		{
			const yafgpu_light &l = sc.lights[0];
			float t = 0.f, ipdf = 0.f;
			const bool ok = arealight_intersect(l, mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), t, ipdf);
			o[0] = ok ? 1.f : 0.f; o[1] = ok ? t : 0.f; o[2] = ok ? ipdf : 0.f;
			o[3] = ok ? l.color[0] : 0.f; o[4] = ok ? l.color[1] : 0.f; o[5] = ok ? l.color[2] : 0.f;
			break;
		}
		case 10:
		{
			const yafgpu_light &l = sc.lights[1];
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f;
			pointlight_illuminate(l, mk(x[0], x[1], x[2]), c, d, tmax);
			o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = tmax; o[4] = c.r; o[5] = c.g; o[6] = c.b;
			break;
		}
		case 11:
		{	// x = material index, n, ng, wo, wl, s1, s2, sample flags
			const yafgpu_material &m = sc.mats[__float_as_uint(x[0])];
			SurfPt sp; sp.n = mk(x[1], x[2], x[3]); sp.ng = mk(x[4], x[5], x[6]); sp.p = mk(0.f, 0.f, 0.f); sp.mat = 0;
			create_cs(sp.n, sp.nu, sp.nv);
			const V3 wo = mk(x[7], x[8], x[9]), wl = mk(x[10], x[11], x[12]);
			if(m.type == YAFGPU_MAT_BLEND)
			{	// a blend's record, with its constant and its sub-materials' records as the table has them (blend_plain): the same outputs from
				// BlendMaterial's functions, on the surface point as given (initBsdf's lerp of the frame is the vertex code's, wf_mat_hit)
				BlendScratch b; blend_plain(sc.mats, m, b);
				const Col e = blend_eval(b, sp, wo, wl, kAll);
				const float pdf = blend_pdf(b, sp, wo, wl, kGlossy | kDiffuse | kDispersive | kReflect | kTransmit);
				BsdfSample bs; bs.s_1 = x[13]; bs.s_2 = x[14]; bs.pdf = 0.f; bs.flags = __float_as_uint(x[15]); bs.sampled = kNone;
				V3 wi = mk(0.f, 0.f, 0.f); float w = 0.f;
				const Col sc_ = blend_sample(b, sp, wo, wi, bs, w);
				o[0] = __uint_as_float(m.bsdf_flags); o[1] = e.r; o[2] = e.g; o[3] = e.b; o[4] = pdf; o[5] = __uint_as_float(bs.sampled);
				o[6] = sc_.r; o[7] = sc_.g; o[8] = sc_.b; o[9] = wi.x; o[10] = wi.y; o[11] = wi.z; o[12] = bs.pdf; o[13] = w;
				const Col em = blend_emit(b, sp, wo, x[15] != 0.f);
				o[14] = em.r; o[15] = em.g; o[16] = em.b;
				break;
			}
			BsdfDat d;
			const uint32_t fl = mat_init_bsdf(m, d);
			const Col e = mat_eval(m, d, sp, wo, wl, kAll);
			const float pdf = mat_pdf(m, d, sp, wo, wl, kGlossy | kDiffuse | kDispersive | kReflect | kTransmit);
			BsdfSample bs; bs.s_1 = x[13]; bs.s_2 = x[14]; bs.pdf = 0.f; bs.flags = __float_as_uint(x[15]); bs.sampled = kNone;
			V3 wi = mk(0.f, 0.f, 0.f); float w = 0.f;
			const Col sc_ = mat_sample(m, d, sp, wo, wi, bs, w);
			o[0] = __uint_as_float(fl); o[1] = e.r; o[2] = e.g; o[3] = e.b; o[4] = pdf; o[5] = __uint_as_float(bs.sampled);
			o[6] = sc_.r; o[7] = sc_.g; o[8] = sc_.b; o[9] = wi.x; o[10] = wi.y; o[11] = wi.z; o[12] = bs.pdf; o[13] = w;
			const Col em = mat_emit(m, sp, wo, x[15] != 0.f);
			o[14] = em.r; o[15] = em.g; o[16] = em.b;
			break;
		}
		case 12:
		{	// Material::getSpecular + getAlpha: x = material index, n, ng, wo
			const yafgpu_material &m = sc.mats[__float_as_uint(x[0])];
			SurfPt sp; sp.n = mk(x[1], x[2], x[3]); sp.ng = mk(x[4], x[5], x[6]); sp.p = mk(0.f, 0.f, 0.f); sp.mat = 0;
			create_cs(sp.n, sp.nu, sp.nv);
			const V3 wo = mk(x[7], x[8], x[9]);
			if(m.type == YAFGPU_MAT_BLEND)
			{	// (a blend's record: as in op 11)
				BlendScratch b; blend_plain(sc.mats, m, b);
				bool refl, refr; V3 d0, d1; Col c0, c1;
				blend_get_specular(b, sp, wo, (n_in >= 11) ? (int)x[10] : 1, refl, refr, d0, c0, d1, c1);
				o[0] = __uint_as_float((refl ? 1u : 0u) | (refr ? 2u : 0u));
				o[1] = d0.x; o[2] = d0.y; o[3] = d0.z; o[4] = c0.r; o[5] = c0.g; o[6] = c0.b;
				o[7] = d1.x; o[8] = d1.y; o[9] = d1.z; o[10] = c1.r; o[11] = c1.g; o[12] = c1.b;
				o[13] = blend_alpha(b, sp, wo);
				const Col tr = blend_transparency(b, sp, wo);
				o[14] = tr.r; o[15] = tr.g; o[16] = tr.b;
				break;
			}
			BsdfDat d;
			mat_init_bsdf(m, d);
			bool refl, refr; V3 d0, d1; Col c0, c1;
			mat_get_specular(m, d, sp, wo, (n_in >= 11) ? (int)x[10] : 1, refl, refr, d0, c0, d1, c1);
			o[0] = __uint_as_float((refl ? 1u : 0u) | (refr ? 2u : 0u));
			o[1] = d0.x; o[2] = d0.y; o[3] = d0.z; o[4] = c0.r; o[5] = c0.g; o[6] = c0.b;
			o[7] = d1.x; o[8] = d1.y; o[9] = d1.z; o[10] = c1.r; o[11] = c1.g; o[12] = c1.b;
			o[13] = mat_alpha(m, d, sp, wo);
			const Col tr = mat_transparency(m, sp, wo);
			o[14] = tr.r; o[15] = tr.g; o[16] = tr.b;
			break;
		}
		case 13:
		{	// image texture lookup: in (p.xyz, texture index) -> getColor rgba, getFloat
			const int ti = (int)__float_as_uint(x[3]);
			if(sc.tex.nodes == nullptr && sc.tex.textures == nullptr) break;
			if(ti < 0 || ti >= sc.tex.n_textures) break;
			const Rgba4 c = tex_get_color(sc.tex, sc.tex.textures[ti], mk(x[0], x[1], x[2]));
			o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = c.a; o[4] = tex_get_float(sc.tex, sc.tex.textures[ti], mk(x[0], x[1], x[2]));
			break;
		}
		case 14:
		{	// node stack of material x[18] at a surface point (p, n, ng, orco_p, orco_ng, u, v): n_nodes x (rgba, scalar); one node
			// range at a time (x[19] = first node of the range, x[20] = count <= kMaxNodes) so that graphs larger than a material's
			// limit can be pinned piecewise by tests that arrange the ranges to be closed under dependencies
			if(sc.tex.nodes == nullptr) break;
			TexPoint tp;
			tp.p = mk(x[0], x[1], x[2]); tp.n = mk(x[3], x[4], x[5]); tp.ng = mk(x[6], x[7], x[8]);
			tp.orco_p = mk(x[9], x[10], x[11]); tp.orco_ng = mk(x[12], x[13], x[14]); tp.u = x[15]; tp.v = x[16];
			const int first = (int)__float_as_uint(x[18]), cnt = min((int)__float_as_uint(x[19]), kMaxNodes);
			NodeResult stack[kMaxNodes];
			nodes_eval(sc.tex, sc.tex.nodes + first, cnt, sc.cam, tp, stack);
			for(int k = 0; k < cnt && 5 * k + 4 < n_out; ++k) { o[5 * k] = stack[k].col.r; o[5 * k + 1] = stack[k].col.g; o[5 * k + 2] = stack[k].col.b; o[5 * k + 3] = stack[k].col.a; o[5 * k + 4] = stack[k].f; }
			break;
		}
		case 15:
		{	// bump mapping: evalDerivative of a node range at a surface point — op 14's 20 words with x[17] = the scale applied to the last
			// node's derivative, then ds_du, ds_dv, nu, nv, has_uv: n_nodes x (du, dv, 0, alpha, f), then (out + 5 * cnt) n, nu, nv after applyBump
			if(sc.tex.nodes == nullptr || n_in < 33) break;
			TexPoint tp;
			tp.p = mk(x[0], x[1], x[2]); tp.n = mk(x[3], x[4], x[5]); tp.ng = mk(x[6], x[7], x[8]);
			tp.orco_p = mk(x[9], x[10], x[11]); tp.orco_ng = mk(x[12], x[13], x[14]); tp.u = x[15]; tp.v = x[16];
			tp.ds_du = mk(x[20], x[21], x[22]); tp.ds_dv = mk(x[23], x[24], x[25]); tp.nu = mk(x[26], x[27], x[28]); tp.nv = mk(x[29], x[30], x[31]);
			tp.has_uv = x[32] != 0.f;
			const int first = (int)__float_as_uint(x[18]), cnt = min((int)__float_as_uint(x[19]), kMaxNodes);
			NodeResult stack[kMaxNodes];
			nodes_eval_derivative(sc.tex, sc.tex.nodes + first, cnt, sc.cam, tp, stack);
			for(int k = 0; k < cnt && 5 * k + 4 < n_out; ++k) { o[5 * k] = stack[k].col.r; o[5 * k + 1] = stack[k].col.g; o[5 * k + 2] = stack[k].col.b; o[5 * k + 3] = stack[k].col.a; o[5 * k + 4] = stack[k].f; }
			if(cnt > 0 && 5 * cnt + 9 <= n_out)
			{
				V3 n = tp.n, nu = tp.nu, nv = tp.nv;
				apply_bump(n, nu, nv, stack[cnt - 1].col.r * x[17], stack[cnt - 1].col.g * x[17]);
				float *q = o + 5 * cnt;
				q[0] = n.x; q[1] = n.y; q[2] = n.z; q[3] = nu.x; q[4] = nu.y; q[5] = nu.z; q[6] = nv.x; q[7] = nv.y; q[8] = nv.z;
			}
			break;
		}
		case 16:
		{	// the two-direction Material::sample of recursiveRaytrace's glossy branch (rough glass): op 11's 16 words in,
			// dir[0], ret, w[0], dir[1], tcol, w[1], pdf, sampled flags out
			const yafgpu_material &m = sc.mats[__float_as_uint(x[0])];
			if(m.type != YAFGPU_MAT_ROUGH_GLASS || n_out < 16) break;
			SurfPt sp; sp.n = mk(x[1], x[2], x[3]); sp.ng = mk(x[4], x[5], x[6]); sp.p = mk(0.f, 0.f, 0.f); sp.mat = 0;
			create_cs(sp.n, sp.nu, sp.nv);
			const V3 wo = mk(x[7], x[8], x[9]);
			BsdfSample bs; bs.s_1 = x[13]; bs.s_2 = x[14]; bs.pdf = 0.f; bs.flags = __float_as_uint(x[15]); bs.sampled = kNone;
			V3 d0 = mk(0.f, 0.f, 0.f), d1 = d0; Col tcol = mkc(0.f, 0.f, 0.f); float w0 = 0.f, w1 = 0.f;
			const Col ret = rough_glass_sample(m, sp, wo, bs, true, d0, w0, d1, tcol, w1);
			o[0] = d0.x; o[1] = d0.y; o[2] = d0.z; o[3] = ret.r; o[4] = ret.g; o[5] = ret.b; o[6] = w0;
			o[7] = d1.x; o[8] = d1.y; o[9] = d1.z; o[10] = tcol.r; o[11] = tcol.g; o[12] = tcol.b; o[13] = w1; o[14] = bs.pdf; o[15] = __uint_as_float(bs.sampled);
			break;
		}
		// the directional, sun and sphere lights (ops 17-21): the light is sc.lights[k], k the last input word (a uint's bits); a k that is out of
		// range or names a light of another type leaves the outputs at zero
		case 17:
		{	// DirectionalLight::illuminate: in p.xyz, k -> ok, wi.dir, wi.tmax, col
			if(n_in < 4) break;
			const uint32_t k = __float_as_uint(x[3]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_DIRECTIONAL || n_out < 8) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f;
			const bool ok = directionallight_illuminate(sc.lights[k], mk(x[0], x[1], x[2]), c, d, tmax);
			o[0] = ok ? 1.f : 0.f;
			o[1] = ok ? d.x : 0.f; o[2] = ok ? d.y : 0.f; o[3] = ok ? d.z : 0.f; o[4] = ok ? tmax : 0.f; o[5] = ok ? c.r : 0.f; o[6] = ok ? c.g : 0.f; o[7] = ok ? c.b : 0.f;
			break;
		}
		case 18:
		{	// SunLight::illumSample: in s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col
			if(n_in < 3) break;
			const uint32_t k = __float_as_uint(x[2]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_SUN || n_out < 9) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f;
			const bool ok = sunlight_illum_sample(sc.lights[k], x[0], x[1], d, tmax, pdf, c);
			o[0] = ok ? 1.f : 0.f;
			o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = c.r; o[7] = c.g; o[8] = c.b;
			break;
		}
		case 19:
		{	// SunLight::intersect: in dir.xyz, k -> ok, t, ipdf, col
			if(n_in < 4) break;
			const uint32_t k = __float_as_uint(x[3]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_SUN || n_out < 6) break;
			Col c = mkc(0.f, 0.f, 0.f); float t = 0.f, ipdf = 0.f;
			const bool ok = sunlight_intersect(sc.lights[k], mk(x[0], x[1], x[2]), t, c, ipdf);
			o[0] = ok ? 1.f : 0.f; o[1] = t; o[2] = ipdf; o[3] = c.r; o[4] = c.g; o[5] = c.b;
			break;
		}
		case 20:
		{	// SphereLight::illumSample: in p.xyz, s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col
			if(n_in < 6) break;
			const uint32_t k = __float_as_uint(x[5]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_SPHERE || n_out < 9) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f;
			const bool ok = spherelight_illum_sample(sc.lights[k], mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf, c);
			o[0] = ok ? 1.f : 0.f;
			o[1] = ok ? d.x : 0.f; o[2] = ok ? d.y : 0.f; o[3] = ok ? d.z : 0.f; o[4] = ok ? tmax : 0.f; o[5] = ok ? pdf : 0.f;
			o[6] = ok ? c.r : 0.f; o[7] = ok ? c.g : 0.f; o[8] = ok ? c.b : 0.f;
			break;
		}
		case 21:
		{	// sphereIntersect__ against sphere light k's center and squared radius: in from.xyz, dir.xyz, k -> ret, d_1, d_2 (d_2 only on a hit)
			if(n_in < 7) break;
			const uint32_t k = __float_as_uint(x[6]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_SPHERE || n_out < 3) break;
			float d_1 = 0.f, d_2 = 0.f;
			const bool ok = sphere_intersect(mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), vec3(sc.lights[k].position), sc.lights[k].square_radius, d_1, d_2);
			o[0] = ok ? 1.f : 0.f; o[1] = d_1; o[2] = ok ? d_2 : 0.f;
			break;
		}
		case 22:
		{	// Background::eval: in dir.xyz -> rgb
			if(n_in < 3 || n_out < 3 || sc.bg.rec.kind == YAFGPU_BACKGROUND_NONE) break;
			const Col c = bg_eval<true>(sc.bg, sc.tex, mk(x[0], x[1], x[2]));      // (<true>: with the skies' code, which this unit's wf_shade is built without)
			o[0] = c.r; o[1] = c.g; o[2] = c.b;
			break;
		}
		case 23:
		{	// BackgroundLight::illumSample: in s_1, s_2 -> ok, wi.dir, wi.tmax, pdf, ls.col
			if(n_in < 2 || n_out < 9 || sc.bg.tab == nullptr) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f;
			const bool ok = bglight_illum_sample<true>(sc.bg, sc.tex, x[0], x[1], d, tmax, pdf, c);
			o[0] = ok ? 1.f : 0.f;
			o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = c.r; o[7] = c.g; o[8] = c.b;
			break;
		}
		case 24:
		{	// BackgroundLight::intersect of the scene's background light: in dir.xyz -> ok, t, ipdf, col
			if(n_in < 3 || n_out < 6 || sc.bg.tab == nullptr) break;
			int k = 0;
			while(k < sc.n_lights && sc.lights[k].type != YAFGPU_LIGHT_BACKGROUND) ++k;
			if(k >= sc.n_lights) break;
			Col c = mkc(0.f, 0.f, 0.f); float t = 0.f, ipdf = 0.f;
			const bool ok = bglight_intersect<true>(sc.lights[k], sc.bg, sc.tex, mk(x[0], x[1], x[2]), t, c, ipdf);
			o[0] = ok ? 1.f : 0.f; o[1] = t; o[2] = ipdf; o[3] = c.r; o[4] = c.g; o[5] = c.b;
			break;
		}
		case 25:
		{	// the background light's tables: in y (as bits; y = kBgRows reads v_dist_) -> count, integral, 1 / integral, 1 / count, func_ (kBgMaxU), cdf_ (kBgMaxU + 1)
			if(n_in < 1 || sc.bg.tab == nullptr) break;
			const uint32_t y = __float_as_uint(x[0]);
			if(y > (uint32_t)kBgRows) break;
			const float *row = sc.bg.tab + (size_t)y * kBgRowStride;
			for(int k = 0; k < min(n_out, kBgCdf + kBgMaxU + 1); ++k) o[k] = row[k];
			break;
		}
		case 26:
		{	// ao_candidate, one sample of sampleAmbientOcclusion: in material index, p, n, ng, wo, s_1, s_2, shadow bias auto (0 / 1), shadow bias,
			// AO distance, AO colour, then for a material with shader nodes or bump the triangle (as bits) and its barycentrics u, v
			// -> wanted, ray direction, tmin, tmax, contribution, emit() * pdf
			if(n_in < 21 || n_out < 12) break;
			const uint32_t k = __float_as_uint(x[0]);
			if(k >= (uint32_t)sc.n_mats) break;
			SurfPt sp; make_sp(mk(x[1], x[2], x[3]), mk(x[4], x[5], x[6]), mk(x[7], x[8], x[9]), (int)k, sp);
			const V3 wo = mk(x[10], x[11], x[12]);
			yafgpu_material m_tmp;
			const yafgpu_material *mp = &sc.mats[k];
			if(n_in >= 24 && (mp->n_nodes > 0 || mp->n_bump > 0))
			{	// the vertex as st_after_closest makes it: the record a mask picks, the bumped frame, then the material its nodes resolve to there
				const uint32_t tri = __float_as_uint(x[21]);
				if(tri >= (uint32_t)sc.n_tris) break;
				wf_mask_hit(sc, sp, (int)tri, x[22], x[23]);
				mp = &sc.mats[sp.mat];
				wf_bump_hit(sc, sp, (int)tri, x[22], x[23]);
				mp = &wf_mat_hit(sc, sp, (int)tri, x[22], x[23], m_tmp);
			}
			BsdfDat d;
			const uint32_t fl = mat_init_bsdf(*mp, d);
			AoParams ao; ao.bias_auto = x[15] != 0.f ? 1 : 0; ao.shadow_bias = x[16]; ao.dist = x[17]; ao.col = mkc(x[18], x[19], x[20]);
			V3 dir; float tmin, tmax; Col contrib, emit;
			const bool go = ao_candidate(ao, x[13], x[14], sp, *mp, d, fl, wo, true, dir, tmin, tmax, contrib, emit);
			o[0] = go ? 1.f : 0.f; o[1] = dir.x; o[2] = dir.y; o[3] = dir.z; o[4] = tmin; o[5] = tmax;
			o[6] = contrib.r; o[7] = contrib.g; o[8] = contrib.b; o[9] = emit.r; o[10] = emit.g; o[11] = emit.b;
			break;
		}
		case 27:
		{	// the mask material's selection (mask_value / mask_select / wf_mask_hit): in material index, triangle (both as bits), barycentrics u, v,
			// p, n, ng -> the mask scalar, the choice under threshold_ (0 / 1), the choice under 0.5, the index the vertex gets (as bits)
			if(n_in < 13 || n_out < 4 || sc.tex.nodes == nullptr) break;
			const uint32_t k = __float_as_uint(x[0]), tri = __float_as_uint(x[1]);
			if(k >= (uint32_t)sc.n_mats || tri >= (uint32_t)sc.n_tris) break;
			const yafgpu_material &m = sc.mats[k];
			SurfPt sp; make_sp(mk(x[4], x[5], x[6]), mk(x[7], x[8], x[9]), mk(x[10], x[11], x[12]), (int)k, sp);
			wf_mask_hit(sc, sp, (int)tri, x[2], x[3]);
			o[3] = __uint_as_float((uint32_t)sp.mat);
			if(m.type != YAFGPU_MAT_MASKED) break;
			o[0] = mask_value(sc.tex, sc.cam, m, (int)tri, x[2], x[3], sp.p, sp.n, sp.ng);
			o[1] = mask_select(sc.tex, sc.cam, m, (int)tri, x[2], x[3], sp.p, sp.n, sp.ng, false) == m.c_index[1] ? 1.f : 0.f;
			o[2] = mask_select(sc.tex, sc.cam, m, (int)tri, x[2], x[3], sp.p, sp.n, sp.ng, true) == m.c_index[1] ? 1.f : 0.f;
			break;
		}
		case 28:
		{	// the rows the device holds for a triangle: in the triangle index (as bits) -> 44 floats: the three float4 records [0, 12), the
			// geometric normal with the smooth flag [12, 16), the three vertex-normal records [16, 28), the six UV floats [28, 34), the nine
			// orco floats [34, 43), and at [43] which of the optional arrays the scene has (as bits: 1 vertex normals, 2 UVs, 4 orcos;
			// an array it has not reads as zeros)
			if(n_in < 1 || n_out < 44) break;
			const uint32_t tri = __float_as_uint(x[0]);
			if(tri >= (uint32_t)sc.n_tris) break;
			for(int r = 0; r < 3; ++r) { const float4 q = sc.tri[3 * (size_t)tri + (size_t)r]; o[4 * r] = q.x; o[4 * r + 1] = q.y; o[4 * r + 2] = q.z; o[4 * r + 3] = q.w; }
			{ const float4 q = sc.tri_ng[tri]; o[12] = q.x; o[13] = q.y; o[14] = q.z; o[15] = q.w; }
			uint32_t have = 0u;
			if(sc.tri_vn != nullptr)
			{
				have |= 1u;
				for(int r = 0; r < 3; ++r) { const float4 q = sc.tri_vn[3 * (size_t)tri + (size_t)r]; o[16 + 4 * r] = q.x; o[17 + 4 * r] = q.y; o[18 + 4 * r] = q.z; o[19 + 4 * r] = q.w; }
			}
			if(sc.tex.tri_uv != nullptr) { have |= 2u; for(int k = 0; k < 6; ++k) o[28 + k] = sc.tex.tri_uv[6 * (size_t)tri + (size_t)k]; }
			if(sc.tex.tri_orco != nullptr) { have |= 4u; for(int k = 0; k < 9; ++k) o[34 + k] = sc.tex.tri_orco[9 * (size_t)tri + (size_t)k]; }
			o[43] = __uint_as_float(have);
			break;
		}
		case 29:
		{	// Triangle::intersect on the scene's own 48-byte record: in the triangle index (as bits), from.xyz, dir.xyz -> ok, t, u, v of tri_test
			// (zeros where it rejects), then ok, t, u, v of tri_test_flat (as computed, also where it rejects: inf / NaN may stand there)
			if(n_in < 7 || n_out < 8) break;
			const uint32_t tri = __float_as_uint(x[0]);
			if(tri >= (uint32_t)sc.n_tris) break;
			const float4 r0 = sc.tri[3 * (size_t)tri], r1 = sc.tri[3 * (size_t)tri + 1], r2 = sc.tri[3 * (size_t)tri + 2];
			const V3 from = mk(x[1], x[2], x[3]), dir = mk(x[4], x[5], x[6]);
			float t = 0.f, u = 0.f, v = 0.f;
			const bool ok = tri_test(r0, r1, r2, from, dir, t, u, v);
			o[0] = ok ? 1.f : 0.f; o[1] = ok ? t : 0.f; o[2] = ok ? u : 0.f; o[3] = ok ? v : 0.f;
			float tf = 0.f, uf = 0.f, vf = 0.f;
			const bool ok_flat = tri_test_flat(r0, r1, r2, from, dir, tf, uf, vf);
			o[4] = ok_flat ? 1.f : 0.f; o[5] = tf; o[6] = uf; o[7] = vf;
			break;
		}
		case 30:
		{	// the surface point the vertex code makes (Triangle::getSurface): in the triangle index (as bits), barycentrics bu, bv, p.xyz ->
			// get_surface's n, ng, nu, nv [0, 12) and material index (as bits) [12]; tex_point's orco_p, orco_ng [13, 19), u, v [19, 21) and
			// has_uv (0 / 1) [21]; tex_point_derivatives' ds_du, ds_dv [22, 28) where the scene has bump data, zeros otherwise
			if(n_in < 6 || n_out < 28) break;
			const uint32_t tri = __float_as_uint(x[0]);
			if(tri >= (uint32_t)sc.n_tris) break;
			SurfPt sp; get_surface(sc, (int)tri, mk(x[3], x[4], x[5]), x[1], x[2], sp);
			o[0] = sp.n.x; o[1] = sp.n.y; o[2] = sp.n.z; o[3] = sp.ng.x; o[4] = sp.ng.y; o[5] = sp.ng.z;
			o[6] = sp.nu.x; o[7] = sp.nu.y; o[8] = sp.nu.z; o[9] = sp.nv.x; o[10] = sp.nv.y; o[11] = sp.nv.z;
			o[12] = __uint_as_float((uint32_t)sp.mat);
			TexPoint tp; tex_point(sc.tex, (int)tri, x[1], x[2], sp.p, sp.n, sp.ng, tp);
			o[13] = tp.orco_p.x; o[14] = tp.orco_p.y; o[15] = tp.orco_p.z; o[16] = tp.orco_ng.x; o[17] = tp.orco_ng.y; o[18] = tp.orco_ng.z;
			o[19] = tp.u; o[20] = tp.v; o[21] = tp.has_uv ? 1.f : 0.f;
			if(!sc.tex.has_bump) break;
			const float4 r1 = sc.tri[3 * (size_t)tri + 1], r2 = sc.tri[3 * (size_t)tri + 2];
			tex_point_derivatives(sc.tex, (int)tri, mk(r1.x, r1.y, r1.z), mk(r2.x, r2.y, r2.z), sp.n, sp.nu, sp.nv, tp);
			o[22] = tp.ds_du.x; o[23] = tp.ds_du.y; o[24] = tp.ds_du.z; o[25] = tp.ds_dv.x; o[26] = tp.ds_dv.y; o[27] = tp.ds_dv.z;
			break;
		}
		case 31:
		{	// the shading frame BlendMaterial::initBsdf leaves (blend_lerp_frame, with the record's constant): in the index of a blend's record
			// (as bits), n -> n, nu, nv after the lerp [0, 9), create_cs's nu, nv before it [9, 15), val and ival [15, 17)
			if(n_in < 4 || n_out < 17) break;
			const uint32_t k = __float_as_uint(x[0]);
			if(k >= (uint32_t)sc.n_mats || sc.mats[k].type != YAFGPU_MAT_BLEND) break;
			BlendScratch b; blend_plain(sc.mats, sc.mats[k], b);
			SurfPt sp; make_sp(mk(0.f, 0.f, 0.f), mk(x[1], x[2], x[3]), mk(x[1], x[2], x[3]), (int)k, sp);
			o[9] = sp.nu.x; o[10] = sp.nu.y; o[11] = sp.nu.z; o[12] = sp.nv.x; o[13] = sp.nv.y; o[14] = sp.nv.z;
			blend_lerp_frame(sp, b.ival);
			o[0] = sp.n.x; o[1] = sp.n.y; o[2] = sp.n.z; o[3] = sp.nu.x; o[4] = sp.nu.y; o[5] = sp.nu.z; o[6] = sp.nv.x; o[7] = sp.nv.y; o[8] = sp.nv.z;
			o[15] = b.val; o[16] = b.ival;
			break;
		}
		// the mesh light (ops 32-34): the light is sc.lights[k], k the last input word (a uint's bits); a k that is out of range or names a
		// light of another type leaves the outputs at zero
		case 32:
		{	// MeshLight::illumSample: in p.xyz, s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col (zeros where it refuses)
			if(n_in < 6 || n_out < 9) break;
			const uint32_t k = __float_as_uint(x[5]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_MESH) break;
			const yafgpu_light &l = sc.lights[k];
			V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f;
			if(!meshlight_illum_sample(sc, l, mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = l.color[0]; o[7] = l.color[1]; o[8] = l.color[2];
			break;
		}
		case 33:
		{	// MeshLight::intersect: in from.xyz, dir.xyz, tmin, k -> ok, t, ipdf, col (zeros where it refuses)
			if(n_in < 8 || n_out < 6) break;
			const uint32_t k = __float_as_uint(x[7]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_MESH) break;
			const yafgpu_light &l = sc.lights[k];
			float t = 0.f, ipdf = 0.f;
			if(!meshlight_intersect(sc, l, mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), x[6], t, ipdf)) break;
			o[0] = 1.f; o[1] = t; o[2] = ipdf; o[3] = l.color[0]; o[4] = l.color[1]; o[5] = l.color[2];
			break;
		}
		case 34:
		{	// a mesh light's stored row: in k -> count (as bits), area_, integral_, inv_integral_, then func_ (count) and cdf_ (count + 1), as far as n_out reaches
			if(n_in < 1 || n_out < 4) break;
			const uint32_t k = __float_as_uint(x[0]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_MESH) break;
			const yafgpu_light &l = sc.lights[k];
			const float *row = sc.lgeo + l.mesh_row;
			o[0] = __uint_as_float((uint32_t)l.mesh_count); o[1] = l.area; o[2] = row[0]; o[3] = row[1];
			for(int j = 0; j < min(n_out - 4, 2 * l.mesh_count + 1); ++j) o[4 + j] = row[kLgeoFunc + j];
			break;
		}
		// the portal light (ops 35-37), addressed like the mesh light
		case 35:
		{	// BackgroundPortalLight::illumSample: in p.xyz, s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col (zeros where it refuses)
			if(n_in < 6 || n_out < 9) break;
			const uint32_t k = __float_as_uint(x[5]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_PORTAL) break;
			V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f; Col c = mkc(0.f, 0.f, 0.f);
			if(!portallight_illum_sample<true>(sc, sc.lights[k], mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf, c)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = c.r; o[7] = c.g; o[8] = c.b;
			break;
		}
		case 36:
		{	// BackgroundPortalLight::intersect: in from.xyz, dir.xyz, tmin, k -> ok, t, ipdf, col (zeros where it refuses)
			if(n_in < 8 || n_out < 6) break;
			const uint32_t k = __float_as_uint(x[7]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_PORTAL) break;
			float t = 0.f, ipdf = 0.f; Col c = mkc(0.f, 0.f, 0.f);
			if(!portallight_intersect<true>(sc, sc.lights[k], mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), x[6], t, ipdf, c)) break;
			o[0] = 1.f; o[1] = t; o[2] = ipdf; o[3] = c.r; o[4] = c.g; o[5] = c.b;
			break;
		}
		case 37:
		{	// a portal's stored row: in k -> count (as bits), area_, integral_, inv_integral_, then func_ (count), cdf_ (count + 1), the
			// triangles' normals (4 * count: x y z and the smooth word) and their records (12 * count), as far as n_out reaches
			if(n_in < 1 || n_out < 4) break;
			const uint32_t k = __float_as_uint(x[0]);
			if(k >= (uint32_t)sc.n_lights || sc.lights[k].type != YAFGPU_LIGHT_PORTAL) break;
			const yafgpu_light &l = sc.lights[k];
			const float *row = sc.lgeo + l.mesh_row, *rec = sc.lgeo + l.mesh_first;
			const int n = l.mesh_count;
			o[0] = __uint_as_float((uint32_t)n); o[1] = l.area; o[2] = row[0]; o[3] = row[1];
			const int64_t n_row = 2 * (int64_t)n + 1, n_ng = 4 * (int64_t)n, n_rec = 12 * (int64_t)n;
			const int64_t n_all = n_row + n_ng + n_rec, n_copy = (int64_t)n_out - 4 < n_all ? (int64_t)n_out - 4 : n_all;
			for(int64_t j = 0; j < n_copy; ++j)
				o[4 + j] = j < n_row ? row[kLgeoFunc + j] : j < n_row + n_ng ? rec[n_rec + (j - n_row)] : rec[j - n_row - n_ng];
			break;
		}
		// the IES light (ops 38-40), addressed like the others; either of its two types answers each op
		case 38:
		{	// IesData::getRadiance: in h_ang, v_ang (degrees), k -> ok, the radiance
			if(n_in < 3 || n_out < 2) break;
			const uint32_t k = __float_as_uint(x[2]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_IES && sc.lights[k].type != YAFGPU_LIGHT_IES_SOFT)) break;
			o[0] = 1.f; o[1] = ies_radiance(sc.lights[k], sc.lgeo + sc.lights[k].ies_first, x[0], x[1]);
			break;
		}
		case 39:
		{	// IesLight::illuminate: in p.xyz, k -> ok, wi.dir, wi.tmax, col (zeros where it refuses)
			if(n_in < 4 || n_out < 8) break;
			const uint32_t k = __float_as_uint(x[3]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_IES && sc.lights[k].type != YAFGPU_LIGHT_IES_SOFT)) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f;
			if(!ieslight_illuminate(sc, sc.lights[k], mk(x[0], x[1], x[2]), c, d, tmax)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = c.r; o[6] = c.g; o[7] = c.b;
			break;
		}
		case 40:
		{	// IesLight::illumSample: in p.xyz, s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col (zeros where it refuses)
			if(n_in < 6 || n_out < 9) break;
			const uint32_t k = __float_as_uint(x[5]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_IES && sc.lights[k].type != YAFGPU_LIGHT_IES_SOFT)) break;
			V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f; Col c = mkc(0.f, 0.f, 0.f);
			if(!ieslight_illum_sample(sc, sc.lights[k], mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf, c)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = c.r; o[7] = c.g; o[8] = c.b;
			break;
		}
		// the spot light (ops 41-43), addressed like the others; either of its two types answers each op
		case 41:
		{	// SpotLight::illuminate: in p.xyz, k -> ok, wi.dir, wi.tmax, col (zeros where it refuses)
			if(n_in < 4 || n_out < 8) break;
			const uint32_t k = __float_as_uint(x[3]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_SPOT && sc.lights[k].type != YAFGPU_LIGHT_SPOT_SOFT)) break;
			Col c = mkc(0.f, 0.f, 0.f); V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f;
			if(!spotlight_illuminate(sc.lights[k], mk(x[0], x[1], x[2]), c, d, tmax)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = c.r; o[6] = c.g; o[7] = c.b;
			break;
		}
		case 42:
		{	// SpotLight::illumSample: in p.xyz, s_1, s_2, k -> ok, wi.dir, wi.tmax, pdf, ls.col (zeros where it refuses)
			if(n_in < 6 || n_out < 9) break;
			const uint32_t k = __float_as_uint(x[5]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_SPOT && sc.lights[k].type != YAFGPU_LIGHT_SPOT_SOFT)) break;
			V3 d = mk(0.f, 0.f, 0.f); float tmax = 0.f, pdf = 0.f; Col c = mkc(0.f, 0.f, 0.f);
			if(!spotlight_illum_sample(sc.lights[k], mk(x[0], x[1], x[2]), x[3], x[4], d, tmax, pdf, c)) break;
			o[0] = 1.f; o[1] = d.x; o[2] = d.y; o[3] = d.z; o[4] = tmax; o[5] = pdf; o[6] = c.r; o[7] = c.g; o[8] = c.b;
			break;
		}
		case 43:
		{	// SpotLight::intersect: in from.xyz, dir.xyz, k -> ok, t, ipdf, col (zeros where it refuses)
			if(n_in < 7 || n_out < 6) break;
			const uint32_t k = __float_as_uint(x[6]);
			if(k >= (uint32_t)sc.n_lights || (sc.lights[k].type != YAFGPU_LIGHT_SPOT && sc.lights[k].type != YAFGPU_LIGHT_SPOT_SOFT)) break;
			float t = 0.f, ipdf = 0.f; Col c = mkc(0.f, 0.f, 0.f);
			if(!spotlight_intersect(sc.lights[k], mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), t, c, ipdf)) break;
			o[0] = 1.f; o[1] = t; o[2] = ipdf; o[3] = c.r; o[4] = c.g; o[5] = c.b;
			break;
		}
		default: break;
	}
}

// BackgroundLight::init (light_background.cc:78-120): the background's energy on a latitude-longitude grid, one workgroup per row y.
// The threads evaluate the row's cells; one thread then accumulates the row in index order (pdf1d_build), which is what makes the
// tables the reference's bit for bit.
__global__ __launch_bounds__(kBlock) void bg_rows_kernel(const DevScene sc, float *tab)
{
	const int y = (int)blockIdx.x;
	if(y >= kBgRows) return;
	float *row = tab + (size_t)y * kBgRowStride;
	const float inv = 1.f / (float)kBgRows;
	const float fy = ((float)y + 0.5f) * inv;
	const float sintheta = bg_sin_sample(fy);
	const int nu = min(kBgMaxU, max(1, kBgMinU + (int)(sintheta * (float)(kBgMaxU - kBgMinU))));      // (the bounds only say what the arithmetic already gives)
	const float inu = 1.f / (float)nu;
	for(int xi = (int)threadIdx.x; xi < nu; xi += (int)blockDim.x)
	{
		const float fx = ((float)xi + 0.5f) * inu;
		const Col c = bg_eval<true>(sc.bg, sc.tex, bg_inv_spheremap(fx, fy));
		row[kBgFunc + xi] = ((c.r + c.g + c.b) * 0.333333f) * sintheta;      // Rgb::energy, color.h:58
	}
	__syncthreads();
	if(threadIdx.x == 0) pdf1d_build(row, nu);
}
// v_dist_: the same construction over the rows' integrals (:106, :109); one workgroup, after bg_rows_kernel.
// check (the two skies): a sky can leave latitude rows without energy, whose Pdf1D divides by zero.  The same thread counts the rows whose
// integral is not a finite number above zero into the first spare float behind v_dist_'s cdf_ (bit 16: the total is no such number
// either), where the host reads one word back; the tables themselves are what they would be without the count.
constexpr int kBgFlag = kBgCdf + kBgMaxU + 1;
static_assert(kBgFlag < kBgRowStride, "the row stride leaves a spare float behind cdf_");
YG_DEV bool bg_has_energy(float integral) { return integral > 0.f && integral <= 3.402823466e+38f; }
__global__ __launch_bounds__(kBlock) void bg_vdist_kernel(float *tab, int check)
{
	float *row = tab + (size_t)kBgRows * kBgRowStride;
	for(int y = (int)threadIdx.x; y < kBgRows; y += (int)blockDim.x) row[kBgFunc + y] = tab[(size_t)y * kBgRowStride + 1];
	__syncthreads();
	if(threadIdx.x != 0 || blockIdx.x != 0) return;
	pdf1d_build(row, kBgRows);
	if(!check) return;
	uint32_t bad = 0u;
	for(int y = 0; y < kBgRows; ++y) if(!bg_has_energy(row[kBgFunc + y])) ++bad;
	if(!bg_has_energy(row[1])) bad |= 1u << 16;
	row[kBgFlag] = __uint_as_float(bad);
}

// MeshLight::initIs (light_meshlight.cc:55-73), one workgroup per light of the scene; those of other types have nothing to do.  The threads
// compute the triangles' areas into func_ (Triangle::surfaceArea, triangle.cc:169-179: the 0.5 is a double); one thread then builds cdf_
// over them in index order (Pdf1D's constructor) and sums area_, a double sum of the float areas in the same order.  `lights` is the
// scene's own array: the light's area is written there.
// BackgroundPortalLight::initIs (light_background_portal.cc:58-77) is the same statement for the same members, so the portal's kernel below
// runs the same body.
YG_DEV void lgeo_rows(yafgpu_light *lights, int k, float *lgeo)
{
	const int n = lights[k].mesh_count;
	float *row = lgeo + lights[k].mesh_row, *func = row + kLgeoFunc;
	for(int i = (int)threadIdx.x; i < n; i += (int)blockDim.x)
	{
		const float *q = lgeo + 9 * (size_t)(lights[k].mesh_pool + i);
		const V3 a = vec3(q), edge_1 = vec3(q + 3) - a, edge_2 = vec3(q + 6) - a;
		func[i] = (float)(0.5 * (double)length(cross(edge_1, edge_2)));
	}
	__syncthreads();
	if(threadIdx.x != 0) return;
	double total_area = 0.0;
	for(int i = 0; i < n; ++i) total_area += (double)func[i];
	const float integral = pdf1d_cumulate(func, n, func + n);
	row[0] = integral; row[1] = 1.f / integral;
	lights[k].area = (float)total_area;
}
__global__ __launch_bounds__(kBlock) void meshlight_rows_kernel(yafgpu_light *lights, int n_lights, float *lgeo)
{
	const int k = (int)blockIdx.x;
	if(k >= n_lights || lights[k].type != YAFGPU_LIGHT_MESH) return;
	lgeo_rows(lights, k, lgeo);
}
__global__ __launch_bounds__(kBlock) void portallight_rows_kernel(yafgpu_light *lights, int n_lights, float *lgeo)
{
	const int k = (int)blockIdx.x;
	if(k >= n_lights || lights[k].type != YAFGPU_LIGHT_PORTAL) return;
	lgeo_rows(lights, k, lgeo);
}

// wf_trace's own copy of the triangle records (DevScene::tri_walk, refs_walk): record t goes to position pos[t] with t in the spare
// word of its third float4, and every leaf reference becomes the position of its triangle.  One grid-stride loop over both ranges.
__global__ __launch_bounds__(kBlock) void walk_copy_kernel(const float4 *rec, const uint32_t *pos, uint32_t n_tris, const uint32_t *refs, uint32_t n_refs,
                                                            float4 *tri_walk, uint32_t *refs_walk)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	for(size_t t = i0; t < (size_t)n_tris; t += stride)
	{
		const size_t p = pos[t];
		if(p >= (size_t)n_tris) continue;      // (pos is a permutation of [0, n_tris): never taken)
		const float4 r2 = rec[3 * t + 2];
		tri_walk[3 * p] = rec[3 * t];
		tri_walk[3 * p + 1] = rec[3 * t + 1];
		tri_walk[3 * p + 2] = make_float4(r2.x, r2.y, r2.z, __uint_as_float((uint32_t)t));
	}
	for(size_t i = i0; i < (size_t)n_refs; i += stride)
	{
		const uint32_t t = refs[i];
		refs_walk[i] = t < n_tris ? pos[t] : 0u;      // (a reference is a triangle id: the builders make no other)
	}
}

} // namespace yafgpu

// ================================================================================================
// host side of the narrow ABI
using namespace yafgpu;

static float host_fsin(float x);
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIP_OK(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) return fail(-100, std::string(#expr) + ": " + hipGetErrorString(e_)); } while(0)

// Owning handles of the host side: what a scene or an entry point holds is released when it goes, on every exit path.
// DevMem: a device array.  alloc() is for the temporaries of an entry point; reserve() makes a long-lived buffer large enough and
// never shrinks it.
template<typename T> struct DevMem
{
	T *p = nullptr; size_t cap = 0;      // cap: elements reserve() has made room for
	DevMem() = default;
	DevMem(const DevMem &) = delete; DevMem &operator=(const DevMem &) = delete;
	~DevMem() { if(p) (void)hipFree(p); }
	hipError_t alloc(size_t count) { return hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)); }
	// room for `count` elements; the contents are not kept.  Work enqueued on `stream` may still use the old array: it is waited for
	// before the array is freed.  After a failed allocation the buffer is empty (p == nullptr, cap == 0).
	hipError_t reserve(size_t count, hipStream_t stream)
	{
		if(p && count <= cap) return hipSuccess;
		hipError_t e = hipStreamSynchronize(stream);
		if(e != hipSuccess) return e;
		if(p) (void)hipFree(p);
		p = nullptr; cap = 0;
		if((e = alloc(count)) != hipSuccess) { p = nullptr; return e; }
		cap = count;
		return hipSuccess;
	}
	operator T *() const { return p; }
};
struct Stream      // a non-blocking stream, created on first use
{
	hipStream_t s = nullptr;
	Stream() = default;
	Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
	~Stream() { if(s) (void)hipStreamDestroy(s); }
	hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
	operator hipStream_t() const { return s; }
};
struct Event       // an event, created on first use: for ordering only unless asked to time
{
	hipEvent_t e = nullptr;
	Event() = default;
	Event(const Event &) = delete; Event &operator=(const Event &) = delete;
	~Event() { if(e) (void)hipEventDestroy(e); }
	hipError_t create(unsigned flags = hipEventDisableTiming) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
	operator hipEvent_t() const { return e; }
};

// Everything one pass in flight owns: the wavefront workspace, the side stream of its any-hit launches and — for pass pipelining
// (begin_piped_pass) — the internal stream its path work runs on.  Passes that are not pipelined use set 0 on the caller's stream.
struct WfSet
{
	DevMem<uint32_t> pix_prefix;                     // per-tile pixel prefix of the shard's tile list
	DevMem<float4> state, results;                   // parked path records (recursiveRaytrace frames behind the working records), rgba per path
	DevMem<uint32_t> queues, counts, verdict, pix_xy;
	DevMem<float4> filt;                             // transparent shadows: the filter products of the shadow rays
	uint32_t cap = 0; int frame_recs = 0;            // paths and frame records per path the first five are laid out for (WfArgs::cap is the record stride)
	Stream side; Event fork, join;                   // the any-hit launch of an iteration runs beside the closest-hit one
	Stream stream; Event done, acc; bool acc_set = false;      // pipelining: path work done / film added (recorded on the caller's stream; acc_set: ever)
	DevMem<yafgpu_counters> counters;                // a pipelined pass counts here; the sums reach the caller's block on the caller's stream
	// a set that a pass outgrows is laid out anew for exactly what that pass asks (reserve_workspace); cap_for: `cap` after that
	bool outgrown(uint32_t paths, int recs) const { return paths > cap || recs > frame_recs; }
	uint32_t cap_for(uint32_t paths, int recs) const { return outgrown(paths, recs) ? paths : cap; }
};

struct yafgpu_scene
{
	yafgpu_scene() = default;
	yafgpu_scene(const yafgpu_scene &) = delete; yafgpu_scene &operator=(const yafgpu_scene &) = delete;
	~yafgpu_scene() { for(void *p : allocs) (void)hipFree(p); }      // the scene's device arrays first; then the members go, whatever their order
	DevScene dev{};
	std::vector<void *> allocs;          // the scene's device arrays (upload, scene_alloc)
	KdTree tree;
	yafgpu_tree_info info{};
	std::vector<yafgpu_material> mats;
	std::vector<yafgpu_light> h_lights;
	int n_lights = 0;
	// the tile list of the last launch stays resident; it is re-uploaded only when its key changes
	DevMem<int4> d_tiles;
	std::vector<int4> h_tiles;
	int tile_key[7] = {-1, -1, -1, -1, -1, -1, -1};
	std::vector<uint32_t> h_pix_prefix;
	// Pass pipelining (render_wavefront): consecutive passes that do not depend on each other's film take turns on two internal streams, each
	// with its own set of the wavefront buffers, so that one pass's launch tails are filled by the other's launches; the film is added to
	// on the caller's stream, in call order.
	static constexpr int kPipeMax = 2;      // passes in flight at most
	WfSet sets[kPipeMax];
	Event pipe_sync; bool pipe_prev = false;
	int pipe_next = 0, pass_pipelining = -1;      // -1: by size (plan_pass), 0 / 1: forced (yafgpu_scene_set_pass_pipelining)
	uint32_t mat_mask = 0u;              // bit per YAFGPU_MAT_* present; picks the shading kernel variant
	std::vector<char> mat_used;          // per material record: some triangle refers to it, or a mask in use picks it
	uint32_t light_mask = 0u;            // bit per YAFGPU_LIGHT_* present; a variant must have been built for all of them
	size_t lgeo_floats = 0;              // floats of the light-geometry pool: the mesh lights' and portals' triangles and rows, the portals' records, the IES lights' tables (upload_lights, mesh_light_rows)
	size_t ies_base = 0;                 // where the IES lights' tables start in that pool
	bool has_ies = false;                // some light is an IES light: its tables are in the pool
	bool has_sky = false;                // the background is a gradient or a sunsky: the shading units built with their evaluation
	bool has_volumetric = false;
	int max_add_depth = 0;               // the largest Material::additional_depth_ of the scene: recursion frames beyond raydepth
	bool has_glossy_two = false;         // rough glass: a glossy trajectory sends two rays (the replay's call count)
	bool has_glossy = false;             // some material has a glossy lobe that recursiveRaytrace samples (glossy / coated_glossy with as_diffuse off): 12-record frames
	bool has_aniso = false;              // some material has the anisotropic glossy lobe: the general shading kernel
	bool has_bump = false;               // some material has a bump shader: the shading frame is parked per vertex (records 24 / 25, frame record 12)
	bool has_textures = false;           // some material in use has shader nodes: the general shading kernel, texture coordinates parked per path
	bool has_specular = false, has_transparent = false;
	bool has_blend = false;              // some triangle uses a blend material: the shading kernel built with the blend's code (the "blend" unit), for every pass
	DevMem<float> d_filter_table;
	// serial-state replay tables (WfArgs::replay), per scene: a pass that replays is never pipelined
	DevMem<uint32_t> rp_flags; DevMem<float> rp_p; DevMem<uint8_t> rp_kill, rp_calls; DevMem<uint32_t> rp_base;
	DevMem<uint32_t> rp_seg_begin, rp_seg_seed, rp_seg_total, rp_seg_base, rp_counter;
	DevMem<float4> rp_hits;              // closest-hit answers of the record pass (WfArgs::hit_cache)
	// render targets of the host-film entry points, kept between calls (allocating and freeing 100 MB per render cost up to half a
	// second a call on this runtime — ten times the pass itself at 1024x1024)
	DevMem<float> rt_planes, rt_film; DevMem<yafgpu_counters> rt_cnt;
	int rt_film_w = 0, rt_film_h = 0;    // the frame whose finished film rt_film holds (0: none): what yafgpu_scene_film_to_image converts
	DevMem<uint8_t> rt_image;            // the packed image of the output stage (yafgpu_scene_film_to_image)
	DevMem<uint8_t> rt_flags;            // resample flags of the detection step between adaptive passes
	int n_cus = 0;                                            // compute units of the device the scene lives on
	uint32_t lc_host_counter = 0;                        // correlative_sample_number_ of a sharded render: the same value on every rank (lc_exchange_counts)
	std::vector<uint32_t> h_seg_base;
	std::vector<uint32_t> h_listed;                      // pixels of a masked (adaptive) pass, in tile order
	std::vector<uint32_t> h_seg_begin, h_seg_seed;       // every chunk's segments of the pass, uploaded once (scene-owned: an async copy may read them late)
	yafgpu_exchange_fn exchange = nullptr; void *exchange_user = nullptr;     // yafgpu_scene_set_exchange
	const volatile int32_t *abort_flag = nullptr;      // polled between chunks and passes (yafgpu_scene_set_abort_flag)
	bool aborted() const { return abort_flag && *abort_flag != 0; }
	bool profiling = false;
	double prof_ms[4] = {0, 0, 0, 0}; uint64_t prof_launches[4] = {0, 0, 0, 0};   // trace closest, trace shadow, shade, other
};

template<typename T> static int upload(yafgpu_scene *s, const T *src, size_t n, const T **dst)
{
	void *p = nullptr;
	const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
	HIP_OK(hipMalloc(&p, bytes));
	s->allocs.push_back(p);
	if(n) HIP_OK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
	s->info.device_bytes += bytes;
	*dst = (const T *)p;
	return 0;
}

// ---- instanced geometry and curve meshes (yafgpu_instancing): the scene's rows are made by yafgpu_assemble.hip --------------
// Every range the kernel will index is checked here, on the host, before anything is launched.
// the rows a segment makes: a curve of n points is 6 * (n - 1) + 2 triangles (scene.cc:200-275), the other kinds one per source row
static uint64_t segment_rows(const yafgpu_segment &sg) { return sg.kind == YAFGPU_SEGMENT_CURVE ? 6u * (uint64_t)(sg.count - 1) + 2u : (uint64_t)sg.count; }

static int check_instancing(const yafgpu_scene_desc *d)
{
	const yafgpu_instancing &in = d->inst;
	if(!in.segments) return fail(-1, "instanced geometry: null segment list");
	if(in.n_base_tris < 0) return fail(-3, "instanced geometry: negative base triangle count");
	if(in.n_curve_points < 0 || (in.n_curve_points > 0 && !in.curve_points)) return fail(in.n_curve_points < 0 ? -3 : -1, "instanced geometry: curve point pool without points");
	if(d->n_tris > 0 && (!d->verts || !d->tri_mat)) return fail(-1, "instanced geometry: plain triangles without vertices or materials");
	if(in.n_base_tris > 0 && (!in.base_verts || !in.base_mat)) return fail(-1, "instanced geometry: base triangles without vertices or materials");
	if(in.base_vnormals && !in.base_vn_index0) return fail(-1, "instanced geometry: base vertex normals without their index-0 marks");
	uint64_t total = 0;
	for(int k = 0; k < in.n_segments; ++k)
	{
		const yafgpu_segment &sg = in.segments[k];
		if(sg.kind != YAFGPU_SEGMENT_PLAIN && sg.kind != YAFGPU_SEGMENT_INSTANCE && sg.kind != YAFGPU_SEGMENT_CURVE) return fail(-3, "instanced geometry: segment " + std::to_string(k) + ": unknown kind");
		if(sg.kind == YAFGPU_SEGMENT_CURVE)
		{	// a strand: points of the curve pool, at least two (scene.cc:174 divides by n - 1), one material for all its rows
			if(sg.first < 0 || sg.count < 2 || (int64_t)sg.first + (int64_t)sg.count > (int64_t)in.n_curve_points)
				return fail(-3, "instanced geometry: segment " + std::to_string(k) + ": a curve needs two or more points inside the curve point pool");
			if(sg.flags >= (uint32_t)d->n_materials) return fail(-3, "instanced geometry: segment " + std::to_string(k) + ": curve material index out of range");
			total += segment_rows(sg);
			continue;
		}
		const int64_t room = sg.kind == YAFGPU_SEGMENT_INSTANCE ? in.n_base_tris : d->n_tris;
		if(sg.first < 0 || sg.count < 0 || (int64_t)sg.first + (int64_t)sg.count > room)
			return fail(-3, "instanced geometry: segment " + std::to_string(k) + ": rows outside the " + (sg.kind == YAFGPU_SEGMENT_INSTANCE ? "base pools" : "plain arrays"));
		total += (uint64_t)sg.count;
	}
	for(size_t k = 0; k < (size_t)std::max(in.n_curve_points, 0) * 5; ++k)
		if(!std::isfinite(in.curve_points[k])) return fail(-3, "non-finite coordinate or extrusion scale in curve point " + std::to_string(k / 5));
	if(total > (uint64_t)INT32_MAX / 9u) return fail(-3, "instanced geometry: more than " + std::to_string(INT32_MAX / 9) + " triangles after flattening");
	for(int i = 0; i < in.n_base_tris; ++i)
		if(in.base_mat[i] < 0 || in.base_mat[i] >= d->n_materials) return fail(-3, "base triangle material index out of range");
	for(size_t k = 0; k < (size_t)in.n_base_tris * 9; ++k)
		if(!std::isfinite(in.base_verts[k])) return fail(-3, "non-finite vertex coordinate in base triangle " + std::to_string(k / 9));
	return 0;
}

// A mask picks between, and a blend mixes, two records that are plain materials themselves (neither a mask nor a blend: no nesting); the
// union of flags either carries (material_mask.cc:34) is no lobe of its own, so check_desc's lobe tests are its sub-materials' to pass.
static int check_mask_or_blend(const yafgpu_scene_desc *d, int i)
{
	const yafgpu_material &m = d->materials[i];
	const bool blend = m.type == YAFGPU_MAT_BLEND;
	const std::string kind = blend ? "blend" : "mask", who = kind + " material " + std::to_string(i);
	for(int k = 0; k < 2; ++k)
	{
		const int sub = m.c_index[k];
		const int type = sub < 0 || sub >= d->n_materials ? YAFGPU_MAT_MASKED : d->materials[sub].type;
		if(blend ? (type >= YAFGPU_MAT_MASKED || type < 0) : (type == YAFGPU_MAT_MASKED || type == YAFGPU_MAT_BLEND))
			return fail(-3, who + ": a sub-material index outside the table, or a mask or a blend under a " + kind + " (nesting is not built)");
	}
	// a mask needs its node, of its own range; a blend takes its value from a node or from a constant
	if(blend && (m.n_nodes < 0 || (m.n_nodes > 0 && (!d->nodes || m.sh_diffuse < 0 || m.sh_diffuse >= m.n_nodes)) || m.n_bump != 0))
		return fail(-24, who + ": a blend with nodes needs the blend node among them, and has no bump shader");
	if(!blend && (!d->nodes || m.n_nodes < 1 || m.sh_diffuse < 0 || m.sh_diffuse >= m.n_nodes || m.n_bump != 0))
		return fail(-24, who + ": needs shader nodes and a mask node among them, and has no bump shader");
	for(int k = 0; k < 2 && blend; ++k)
		if(d->materials[m.c_index[k]].n_bump != 0)
			return fail(-24, who + ": a sub-material with a bump shader (BlendMaterial::initBsdf would blend two bumped frames, surface.cc:137-151)");
	// recursiveRaytrace's glossy branch picks its case from the mask's or blend's flags, the union (integrator_montecarlo.cc:895-919): next to a
	// transmitting partner a glossy sub-material lands in the reflect + transmit case, whose two-direction sample MaskMaterial leaves at
	// Material's empty default and BlendMaterial's (material_blend.cc:216-236) is not restated
	const uint32_t both = d->materials[m.c_index[0]].bsdf_flags | d->materials[m.c_index[1]].bsdf_flags;
	if((both & kGlossy) && (both & kReflect) && (both & kTransmit))
		return fail(-4, who + ": a glossy sub-material beside a transmitting one (recursiveRaytrace reads the union of their flags, integrator_montecarlo.cc:895-919)");
	return 0;
}

// Mesh lights: every range the kernels will index — the light's scene rows, its triangles in the light-geometry pool — lies inside its
// array, and the pool's corners are finite.  (After check_instancing: the scene's row count is the segments'.)
static int check_mesh_lights(const yafgpu_scene_desc *d)
{
	int64_t rows = d->n_tris;
	if(d->inst.n_segments > 0) { rows = 0; for(int k = 0; k < d->inst.n_segments; ++k) rows += (int64_t)segment_rows(d->inst.segments[k]); }
	bool any = false;
	for(int i = 0; i < d->n_lights; ++i)
	{
		const yafgpu_light &l = d->lights[i];
		if(l.type != YAFGPU_LIGHT_MESH && l.type != YAFGPU_LIGHT_PORTAL) continue;
		const bool portal = l.type == YAFGPU_LIGHT_PORTAL;
		const std::string who = (portal ? "portal light " : "mesh light ") + std::to_string(i);
		any = true;
		if(l.mesh_count < 1) return fail(-2, who + ": a mesh with no triangles");
		// a portal's triangles have no scene rows; what it asks instead is a background and a material for each of its triangles
		if(portal && d->background.kind == YAFGPU_BACKGROUND_NONE) return fail(-2, who + ": a portal needs a background to take its colour from");
		if(!portal && (l.mesh_first < 0 || (int64_t)l.mesh_first + (int64_t)l.mesh_count > rows)) return fail(-3, who + ": its rows lie outside the scene's triangles");
		if(!d->light_verts || l.mesh_pool < 0 || (int64_t)l.mesh_pool + (int64_t)l.mesh_count > (int64_t)d->n_light_tris)
			return fail(-3, who + ": its triangles lie outside the light-geometry pool");
		if(!portal) continue;
		if(!d->light_tri_mat) return fail(-3, who + ": no materials for the triangles of the light-geometry pool (light_tri_mat)");
		for(int32_t k = l.mesh_pool; k < l.mesh_pool + l.mesh_count; ++k)
			if(d->light_tri_mat[k] < 0 || d->light_tri_mat[k] >= d->n_materials) return fail(-3, who + ": triangle material index out of range");
	}
	if(!any) return 0;
	for(size_t k = 0; k < (size_t)d->n_light_tris * 9; ++k)
		if(!std::isfinite(d->light_verts[k])) return fail(-3, "non-finite vertex coordinate in triangle " + std::to_string(k / 9) + " of the light-geometry pool");
	return 0;
}

// IES lights: the light's two maps and its table lie inside the table pool, the maps are strictly increasing (the lookup divides by their
// steps and bisects them) and max_rad_ is a number to multiply by.
static int check_ies_lights(const yafgpu_scene_desc *d)
{
	for(int i = 0; i < d->n_lights; ++i)
	{
		const yafgpu_light &l = d->lights[i];
		if(l.type != YAFGPU_LIGHT_IES && l.type != YAFGPU_LIGHT_IES_SOFT) continue;
		const std::string who = "IES light " + std::to_string(i);
		if(l.ies_n_hor < 2 || l.ies_n_vert < 2) return fail(-2, who + ": fewer than 2 horizontal or 2 vertical angles");
		const int64_t floats = (int64_t)l.ies_n_hor + (int64_t)l.ies_n_vert + (int64_t)l.ies_n_hor * (int64_t)l.ies_n_vert;
		if(!d->ies_tables || d->n_ies_floats <= 0 || l.ies_first < 0 || (int64_t)l.ies_first + floats > (int64_t)d->n_ies_floats)
			return fail(-3, who + ": its maps and table lie outside the IES table pool");
		const float *hor = d->ies_tables + l.ies_first, *vert = hor + l.ies_n_hor;
		for(int k = 1; k < l.ies_n_hor; ++k) if(!(hor[k] > hor[k - 1])) return fail(-3, who + ": its horizontal angles are not strictly increasing");
		for(int k = 1; k < l.ies_n_vert; ++k) if(!(vert[k] > vert[k - 1])) return fail(-3, who + ": its vertical angles are not strictly increasing");
		if(!(l.ies_max_rad > 0.f && std::isfinite(l.ies_max_rad))) return fail(-3, who + ": max_rad is not finite and positive");
	}
	return 0;
}

// Spot lights: the record indexes nothing, so all there is to hold are its numbers: the two cosines and shadow_fuzzy_ finite, the axis a
// vector of numbers; icos_diff_ may be infinite (blend 0, where the falloff branch is unreachable) but is no NaN.
static int check_spot_lights(const yafgpu_scene_desc *d)
{
	for(int i = 0; i < d->n_lights; ++i)
	{
		const yafgpu_light &l = d->lights[i];
		if(l.type != YAFGPU_LIGHT_SPOT && l.type != YAFGPU_LIGHT_SPOT_SOFT) continue;
		const std::string who = "spot light " + std::to_string(i);
		if(!(std::isfinite(l.cos_angle) && std::isfinite(l.spot_cos_start))) return fail(-3, who + ": the cosines of its cone are not finite");
		if(std::isnan(l.spot_icos_diff)) return fail(-3, who + ": icos_diff is not a number");
		if(!std::isfinite(l.spot_shadow_fuzzy)) return fail(-3, who + ": shadow_fuzzy is not finite");
		for(int k = 0; k < 3; ++k) if(!std::isfinite(l.direction[k])) return fail(-3, who + ": its axis is not finite");
	}
	return 0;
}

// every reference inside a node range is -1 or names a node BEFORE the one that reads it (evaluation order): the device indexes a per-lane
// result stack with them (nodes_eval, mat_resolve, nodes_eval_derivative)
static bool node_range_ok(const yafgpu_node *nodes, int first, int count)
{
	for(int k = 0; k < count; ++k)
	{
		const yafgpu_node &n = nodes[first + k];
		auto ref_ok = [&](int r) { return r >= -1 && r < k; };
		if(n.type == YAFGPU_NODE_MIX && !(ref_ok(n.input1) && ref_ok(n.input2) && ref_ok(n.factor))) return false;
		if(n.type == YAFGPU_NODE_LAYER && !(n.input >= 0 && n.input < k && ref_ok(n.upper))) return false;
		if(n.type < YAFGPU_NODE_TEXTURE_MAPPER || n.type > YAFGPU_NODE_LAYER) return false;
	}
	return true;
}

// Every refusal that depends on the descriptor alone, on the host, before a scene object or any device memory exists.  (One refusal is left
// for later: a coordinate that an instance's matrix overflows, which only the device finds, assemble_scene.)
// the constants of a gradient or a sunsky background, before anything is uploaded: every value the kind reads is a finite number, and a
// sunsky's direction is not the zero vector (its normalisation would leave it zero, and theta_s with it a quarter turn whatever was meant)
static int check_sky(int kind, const yafgpu_sky &k)
{
	if(kind == YAFGPU_BACKGROUND_GRADIENT)
	{
		const float *cols[4] = {k.horizon, k.zenith, k.horizon_ground, k.zenith_ground};
		for(const float *c : cols)
			for(int j = 0; j < 3; ++j)
				if(!std::isfinite(c[j])) return fail(-2, "gradient background: a colour is not finite");
		return 0;
	}
	if(k.from[0] == 0.f && k.from[1] == 0.f && k.from[2] == 0.f) return fail(-2, "sunsky background: `from`, the direction to the sun, is the zero vector");
	const double vals[5] = {k.theta_s, k.phi_s, k.zenith_x, k.zenith_y, k.zenith_Y};
	bool ok = std::isfinite(k.power) && std::isfinite(k.turbidity) && std::isfinite(k.from[0]) && std::isfinite(k.from[1]) && std::isfinite(k.from[2]);
	for(double v : vals) ok = ok && std::isfinite(v);
	for(int j = 0; j < 5; ++j) ok = ok && std::isfinite(k.perez_x[j]) && std::isfinite(k.perez_y[j]) && std::isfinite(k.perez_Y[j]);
	if(!ok) return fail(-2, "sunsky background: a value of the sky record (power, turbidity, from, the sun's angles, the zenith values or a Perez coefficient) is not finite");
	return 0;
}

static int check_desc(const yafgpu_scene_desc *d)
{
	if(!d) return fail(-1, "null argument");
	if(d->n_tris < 0 || d->n_materials <= 0) return fail(-2, "scene needs at least one material");
	// the light-estimate bookkeeping of a parked path packs the light index and the end of its light range in 8 bits each
	// (pack_dlc, yafgpu_wavefront.h)
	if(d->n_lights < 0 || d->n_lights > 255) return fail(-2, "more than 255 lights: the device path indexes lights with 8 bits");
	{	// a NaN or infinite coordinate poisons the scene bound and with it every ray's clip against it: refuse it here
		const size_t nf = (size_t)d->n_tris * 9;
		for(size_t k = 0; k < nf; ++k)
			if(!std::isfinite(d->verts[k])) return fail(-3, "non-finite vertex coordinate in triangle " + std::to_string(k / 9));
	}
	for(int i = 0; i < d->n_tris; ++i)
		if(d->tri_mat[i] < 0 || d->tri_mat[i] >= d->n_materials) return fail(-3, "triangle material index out of range");
	for(int i = 0; i < d->n_lights; ++i)
		if(d->lights[i].type < YAFGPU_LIGHT_AREA || (d->lights[i].type > YAFGPU_LIGHT_BACKGROUND && d->lights[i].type != YAFGPU_LIGHT_MESH && d->lights[i].type != YAFGPU_LIGHT_PORTAL && d->lights[i].type != YAFGPU_LIGHT_IES && d->lights[i].type != YAFGPU_LIGHT_IES_SOFT && d->lights[i].type != YAFGPU_LIGHT_SPOT && d->lights[i].type != YAFGPU_LIGHT_SPOT_SOFT)) return fail(-2, "light " + std::to_string(i) + ": unknown type");
	{	// the background and its light: one record, at most one light, and the light only with a background that asks for it
		const yafgpu_background &b = d->background;
		int n_bg_lights = 0;
		for(int i = 0; i < d->n_lights; ++i) if(d->lights[i].type == YAFGPU_LIGHT_BACKGROUND) ++n_bg_lights;
		const bool sky = b.kind == YAFGPU_BACKGROUND_GRADIENT || b.kind == YAFGPU_BACKGROUND_SUNSKY;
		if((b.kind < YAFGPU_BACKGROUND_NONE || b.kind > YAFGPU_BACKGROUND_TEXTURE) && !sky) return fail(-2, "background: unknown kind");
		if(sky) { const int rc = check_sky(b.kind, d->sky); if(rc) return rc; }
		if(n_bg_lights > 1) return fail(-2, "more than one background light");
		if(n_bg_lights != ((b.kind != YAFGPU_BACKGROUND_NONE && b.has_ibl) ? 1 : 0)) return fail(-2, "a background light needs a background with has_ibl, and such a background its light");
		if(b.kind == YAFGPU_BACKGROUND_TEXTURE)
		{
			if(!d->textures || b.texture < 0 || b.texture >= d->n_textures) return fail(-24, "the background's texture does not exist");
			if(b.projection != 0 && b.projection != 1) return fail(-2, "background: unknown projection");
		}
		if(b.kind == YAFGPU_BACKGROUND_CONSTANT && b.has_ibl && !((b.color[0] + b.color[1] + b.color[2]) * 0.333333f > 0.f))
			return fail(-2, "a constant background with a light needs a colour with energy (Pdf1D would divide by zero)");
	}
	for(int i = 0; i < d->n_materials; ++i)
	{
		// recursiveRaytrace (integrator_montecarlo.cc:782-1028): the perfect specular branch and both cases of the glossy branch (reflect
		// only; reflect + transmit, which is rough glass and nothing else) are on the device path; the dispersive branch is not
		const yafgpu_material &m = d->materials[i];
		if(m.type < 0 || m.type > YAFGPU_MAT_BLEND) return fail(-3, "material " + std::to_string(i) + ": unknown type");
		if(m.type == YAFGPU_MAT_BLEND || m.type == YAFGPU_MAT_MASKED)
		{
			const int rc = check_mask_or_blend(d, i);
			if(rc) return rc;
			continue;
		}
		if(m.bsdf_flags & kDispersive)
			return fail(-4, "material with a dispersive lobe needs recursiveRaytrace's dispersive branch, which the GPU path does not implement");
		if((m.bsdf_flags & kGlossy) && (m.bsdf_flags & kTransmit) && m.type != YAFGPU_MAT_ROUGH_GLASS)
			return fail(-4, "a glossy transmission lobe on a material that is not rough glass: the reflect + transmit case of recursiveRaytrace's glossy branch takes RoughGlassMaterial's two-direction sample");
		if(m.type == YAFGPU_MAT_ROUGH_GLASS && !(m.rg_a2 > 0.f))
			return fail(-3, "rough glass material " + std::to_string(i) + ": rg_a2 (alpha squared) must be positive");
	}
	if(d->inst.n_segments > 0) { const int rc = check_instancing(d); if(rc) return rc; }
	{ const int rc = check_mesh_lights(d); if(rc) return rc; }
	{ const int rc = check_ies_lights(d); if(rc) return rc; }
	{ const int rc = check_spot_lights(d); if(rc) return rc; }
	const bool with_nodes = d->n_nodes > 0 && d->nodes;
	if(with_nodes || d->background.kind == YAFGPU_BACKGROUND_TEXTURE)      // image textures: what the shader nodes and a texture background look up
		for(int i = 0; i < d->n_textures; ++i)
		{
			const yafgpu_texture &t = d->textures[i];
			if(t.width <= 0 || t.height <= 0 || (uint64_t)t.texel_first + (uint64_t)t.width * (uint64_t)t.height > d->n_texels) return fail(-24, "a texture's texel range lies outside the texel array");
		}
	if(!with_nodes) return 0;
	for(int i = 0; i < d->n_materials; ++i)
	{
		const yafgpu_material &m = d->materials[i];
		if(m.n_nodes < 0 || m.n_nodes > kMaxNodes || m.node_first < 0 || m.node_first + m.n_nodes > d->n_nodes)
			return fail(-24, "a material's shader nodes: more than " + std::to_string(kMaxNodes) + " nodes, or a range outside the node array");
		if(m.n_bump < 0 || m.n_bump > kMaxNodes || (m.n_bump > 0 && (m.bump_first < 0 || m.bump_first + m.n_bump > d->n_nodes || m.sh_bump < 0 || m.sh_bump >= m.n_bump)))
			return fail(-24, "a material's bump shader: more than " + std::to_string(kMaxNodes) + " nodes, or a range outside the node array");
		const int slots[] = {m.sh_diffuse, m.sh_mirror_color, m.sh_mirror, m.sh_transparency, m.sh_translucency, m.sh_sigma_oren, m.sh_diffuse_refl, m.sh_ior,
		                     m.sh_glossy, m.sh_glossy_reflect, m.sh_exponent, m.sh_filter_color};
		for(int sl : slots)
			if(m.n_nodes > 0 && (sl < -1 || sl >= m.n_nodes)) return fail(-24, "a material's shader slot names a node outside its node range");
		if(!node_range_ok(d->nodes, m.node_first, m.n_nodes) || (m.n_bump > 0 && !node_range_ok(d->nodes, m.bump_first, m.n_bump)))
			return fail(-24, "a shader node refers to a node that is not evaluated before it (or has an unknown type; a layer needs an input)");
	}
	for(int i = 0; i < d->n_nodes; ++i)
		if(d->nodes[i].type == YAFGPU_NODE_TEXTURE_MAPPER && (d->nodes[i].texture < 0 || d->nodes[i].texture >= d->n_textures)) return fail(-24, "a texture_mapper node refers to a texture that does not exist");
	return 0;
}

// What the scene's materials ask of the pipeline — recursion frames, the glossy loop's wider frames, extra depth, the transparent-shadow
// kernel, the kernel variant — is taken from the materials some triangle actually USES: a definition nothing refers to can never be
// hit, and must not cost frames, a kernel variant or (through the size of the replay's event tables) the exactness of the serial state.
// A mask material in use stands for the two records it picks from: those count, the mask's own type and union of flags do not (it is
// never a vertex's material).  A mask nothing refers to sizes nothing either, and neither do its records.
static void classify_materials(yafgpu_scene *s, const yafgpu_scene_desc *d)
{
	std::vector<char> &used = s->mat_used;
	used.assign((size_t)d->n_materials, 0);
	if(d->inst.n_segments <= 0) for(int i = 0; i < d->n_tris; ++i) used[(size_t)d->tri_mat[i]] = 1;
	for(int k = 0; k < d->inst.n_segments; ++k)
	{	// the rows some segment makes a triangle of
		const yafgpu_segment &sg = d->inst.segments[k];
		if(sg.kind == YAFGPU_SEGMENT_CURVE) { used[(size_t)sg.flags] = 1; continue; }
		const int32_t *mat = sg.kind == YAFGPU_SEGMENT_INSTANCE ? d->inst.base_mat : d->tri_mat;
		for(int i = sg.first; i < sg.first + sg.count; ++i) used[(size_t)mat[i]] = 1;
	}
	for(int i = 0; i < d->n_materials; ++i)
		if(used[(size_t)i] && (d->materials[i].type == YAFGPU_MAT_MASKED || d->materials[i].type == YAFGPU_MAT_BLEND)) used[(size_t)d->materials[i].c_index[0]] = used[(size_t)d->materials[i].c_index[1]] = 1;
	for(int i = 0; i < d->n_materials; ++i)
	{
		if(!used[(size_t)i] || d->materials[i].type == YAFGPU_MAT_MASKED) continue;
		const yafgpu_material &m = d->materials[i];
		// A blend in use IS a vertex's material: the scene takes the shading kernel built with the blend's code (pick_shade_variant), and
		// the blend's own words size what the integrators read off sp.material_ — the union of flags (recursion frames, the glossy loop:
		// recursiveRaytrace enters on them), the larger additional depth, isTransparent(), the volume handler.  Its two records count
		// with their own types and lobes (the anisotropic lobe, rough glass never: that pair is refused).
		const bool blend = m.type == YAFGPU_MAT_BLEND;
		if(m.bsdf_flags & kVolumetric) s->has_volumetric = true;
		if(m.bsdf_flags & (kSpecular | kFilter)) s->has_specular = true;
		if(m.bsdf_flags & kGlossy) s->has_glossy = true;
		s->max_add_depth = std::max(s->max_add_depth, std::min(std::max(m.additional_depth, 0), 15));
		if(blend) { s->has_blend = true; if(m.is_transparent) s->has_transparent = true; continue; }
		s->mat_mask |= 1u << (uint32_t)m.type;
		if(m.anisotropic) s->has_aniso = true;
		if(m.type == YAFGPU_MAT_ROUGH_GLASS) s->has_glossy_two = true;
		if((m.type == YAFGPU_MAT_SHINYDIFFUSE && m.is_transparent) || ((m.type == YAFGPU_MAT_GLASS || m.type == YAFGPU_MAT_ROUGH_GLASS) && m.fake_shadow)) s->has_transparent = true;
	}
	if(!(d->n_nodes > 0 && d->nodes)) return;
	for(int i = 0; i < d->n_materials; ++i)
	{	// shader nodes: the general shading kernel; a bump shader parks the shading frame too
		const yafgpu_material &m = d->materials[i];
		if(m.n_nodes > 0 && ((m.type != YAFGPU_MAT_MASKED && m.type != YAFGPU_MAT_BLEND) || used[(size_t)i])) s->has_textures = true;      // (a mask or a blend nothing refers to picks no kernel)
		if(m.n_bump > 0) { s->has_textures = true; s->has_bump = true; }
	}
}

// The flattened scene's rows, made by host_rows (plain arrays) or assemble_scene (instanced geometry and curves): device arrays owned by the
// scene (yafgpu_scene::allocs), and the corner vertices on the host for the tree builders
struct AssembledRows
{
	uint32_t n = 0;
	const float4 *rec = nullptr, *ng = nullptr, *vn = nullptr;
	const float *uv = nullptr, *orco = nullptr, *e3 = nullptr;
	const yafgpu_material *mats = nullptr;
	const float *verts = nullptr;      // 9 per row: the descriptor's own, or `made`
	std::vector<float> made;           // what came back from the device (assemble_scene)
	std::vector<float4> h_rec, h_ng, h_vn;      // what host_rows made: on the device after upload_rows, behind the tree
};

template<typename T> static int scene_alloc(yafgpu_scene *s, size_t n, T **dst)
{
	void *p = nullptr;
	const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
	HIP_OK(hipMalloc(&p, bytes));
	s->allocs.push_back(p);
	s->info.device_bytes += bytes;
	*dst = (T *)p;
	return 0;
}
template<typename T> static int temp_upload(DevMem<T> &m, const T *src, size_t n)
{
	if(!src || n == 0) return 0;
	HIP_OK(m.alloc(n));
	HIP_OK(hipMemcpy(m.p, src, n * sizeof(T), hipMemcpyHostToDevice));
	return 0;
}

// out.made: the flattened scene's corner vertices, the only output that comes back (the tree builders and the non-finite check read them)
static int assemble_scene(yafgpu_scene *s, const yafgpu_scene_desc *d, AssembledRows &out)
{
	const yafgpu_instancing &in = d->inst;
	std::vector<float> &h_verts = out.made;
	std::vector<yafgpu_segment> segs; std::vector<uint32_t> first;
	bool smooth_segment = d->vnormals != nullptr;
	for(int k = 0; k < in.n_segments; ++k)
	{
		const yafgpu_segment &sg = in.segments[k];
		if(sg.count == 0) continue;
		first.push_back(out.n); segs.push_back(sg); out.n += (uint32_t)segment_rows(sg);      // check_instancing bounded the sum
		if(sg.kind == YAFGPU_SEGMENT_INSTANCE && (sg.flags & YAFGPU_INSTANCE_SMOOTH) && in.base_vnormals) smooth_segment = true;
	}
	first.push_back(out.n);
	h_verts.assign((size_t)out.n * 9, 0.f);
	int rc = 0;
	if((rc = upload(s, d->materials, (size_t)d->n_materials, &out.mats))) return rc;
	const size_t np = (size_t)d->n_tris, nb = (size_t)in.n_base_tris, n = out.n;
	const bool texcoords = d->n_nodes > 0 && d->nodes;      // what the shader nodes read
	bool bump = false;
	for(int i = 0; i < d->n_materials && texcoords; ++i) if(d->materials[i].n_bump > 0) bump = true;
	DevMem<yafgpu_segment> d_segs; DevMem<uint32_t> d_first;
	DevMem<float> p_verts, p_vn, p_uv, p_orco, b_verts, b_vn, b_uv, b_orco, c_points, d_verts; DevMem<int32_t> p_mat, b_mat; DevMem<uint8_t> b_vn0;
	if((rc = temp_upload(d_segs, segs.data(), segs.size())) || (rc = temp_upload(d_first, first.data(), first.size()))) return rc;
	if((rc = temp_upload(p_verts, d->verts, np * 9)) || (rc = temp_upload(p_mat, d->tri_mat, np)) || (rc = temp_upload(p_vn, d->vnormals, np * 9))) return rc;
	if(texcoords && ((rc = temp_upload(p_uv, d->tri_uv, np * 6)) || (rc = temp_upload(p_orco, d->tri_orco, np * 9)))) return rc;
	if((rc = temp_upload(b_verts, in.base_verts, nb * 9)) || (rc = temp_upload(b_mat, in.base_mat, nb))) return rc;
	if((rc = temp_upload(b_vn, in.base_vnormals, nb * 9)) || (rc = temp_upload(b_vn0, in.base_vn_index0, in.base_vnormals ? nb : 0))) return rc;
	if(texcoords && ((rc = temp_upload(b_uv, in.base_uv, nb * 6)) || (rc = temp_upload(b_orco, in.base_orco, nb * 9)))) return rc;
	if((rc = temp_upload(c_points, in.curve_points, (size_t)in.n_curve_points * 5))) return rc;
	float4 *rec = nullptr, *ng = nullptr, *vn = nullptr; float *uv = nullptr, *orco = nullptr, *e3 = nullptr;
	if((rc = scene_alloc(s, 3 * n, &rec)) || (rc = scene_alloc(s, n, &ng))) return rc;
	if(smooth_segment && (rc = scene_alloc(s, 3 * n, &vn))) return rc;
	if(texcoords && ((rc = scene_alloc(s, 6 * n, &uv)) || (rc = scene_alloc(s, 9 * n, &orco)))) return rc;
	if(bump && (rc = scene_alloc(s, 3 * n, &e3))) return rc;
	HIP_OK(d_verts.alloc(9 * n));
	AssembleArgs a{};
	a.segs = d_segs.p; a.seg_first = d_first.p; a.n_segs = (int)segs.size(); a.n_out = out.n;
	a.p_verts = p_verts.p; a.p_mat = p_mat.p; a.p_vn = p_vn.p; a.p_uv = p_uv.p; a.p_orco = p_orco.p;
	a.b_verts = b_verts.p; a.b_mat = b_mat.p; a.b_vn = b_vn.p; a.b_vn0 = b_vn0.p; a.b_uv = b_uv.p; a.b_orco = b_orco.p;
	a.c_points = c_points.p;
	a.mats = out.mats;
	a.rec = rec; a.ng = ng; a.vn = vn; a.uv = uv; a.orco = orco; a.e3 = e3; a.verts = d_verts.p;
	HIP_OK(assemble_rows(a));
	HIP_OK(hipDeviceSynchronize());
	if(n) HIP_OK(hipMemcpy(h_verts.data(), d_verts.p, 9 * n * sizeof(float), hipMemcpyDeviceToHost));
	// a matrix that overflows a coordinate is refused as a bad vertex is
	for(size_t k = 0; k < h_verts.size(); ++k)
		if(!std::isfinite(h_verts[k])) return fail(-3, "non-finite vertex coordinate in triangle " + std::to_string(k / 9));
	out.rec = rec; out.ng = ng; out.vn = vn; out.uv = uv; out.orco = orco; out.e3 = e3; out.verts = h_verts.data();
	return 0;
}

// The same rows from the plain arrays, on the host.  Triangle records: Triangle::updateIntersectionCachedValues (triangle.h:197-207),
// recNormal (:295-302); yafgpu_assemble.hip makes them by these expressions.
static void host_rows(const yafgpu_scene_desc *d, AssembledRows &out)
{
	const size_t nt = (size_t)d->n_tris;
	std::vector<float4> &rec = out.h_rec, &ng = out.h_ng, &vn = out.h_vn;
	rec.resize(3 * nt); ng.resize(nt);
	bool any_smooth = false;
	for(size_t i = 0; i < nt; ++i)
	{
		const float *v = d->verts + 9 * i;
		const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
		const float l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
		const float l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
		const float eps = (float)((double)0.1f * 0.00005 * (double)std::max(l1, l2));
		const uint32_t mat = (uint32_t)d->tri_mat[i];
		const uint32_t vis = (uint32_t)d->materials[mat].visibility & 3u;
		float mw; const uint32_t packed = mat | (vis << 30); std::memcpy(&mw, &packed, 4);
		rec[3 * i] = make_float4(v[0], v[1], v[2], eps);
		rec[3 * i + 1] = make_float4(e1[0], e1[1], e1[2], mw);
		rec[3 * i + 2] = make_float4(e2[0], e2[1], e2[2], 0.f);
		float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
		float len = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
		if(len != 0.f) { len = 1.0f / std::sqrt(len); n[0] *= len; n[1] *= len; n[2] *= len; }
		bool smooth = false;
		if(d->vnormals)
		{
			const float *q = d->vnormals + 9 * i;
			for(int k = 0; k < 9; ++k) if(q[k] != 0.f) smooth = true;
		}
		float sw; const uint32_t sbits = smooth ? 1u : 0u; std::memcpy(&sw, &sbits, 4);
		ng[i] = make_float4(n[0], n[1], n[2], sw);
		any_smooth |= smooth;
	}
	if(any_smooth)
	{
		vn.resize(3 * nt);
		for(size_t i = 0; i < nt; ++i)
		{
			const float *q = d->vnormals + 9 * i;
			for(int c = 0; c < 3; ++c)
			{
				float x = q[3 * c], y = q[3 * c + 1], z = q[3 * c + 2];
				if(x == 0.f && y == 0.f && z == 0.f) { x = ng[i].x; y = ng[i].y; z = ng[i].z; }
				vn[3 * i + (size_t)c] = make_float4(x, y, z, 0.f);
			}
		}
	}
	out.n = (uint32_t)nt; out.verts = d->verts;
}

// What host_rows made goes to the device once the tree is built (the device builder has the memory to itself, and a process's first HIP
// call is the builder's); rows that assemble_scene made are there already.
static int upload_rows(yafgpu_scene *s, const yafgpu_scene_desc *d, AssembledRows &out)
{
	if(out.rec) return 0;
	const size_t nt = out.n;
	int rc = 0;
	if((rc = upload(s, out.h_rec.data(), out.h_rec.size(), &out.rec)) || (rc = upload(s, out.h_ng.data(), out.h_ng.size(), &out.ng))) return rc;
	if(!out.h_vn.empty() && (rc = upload(s, out.h_vn.data(), out.h_vn.size(), &out.vn))) return rc;
	if((rc = upload(s, d->materials, (size_t)d->n_materials, &out.mats))) return rc;
	if(!(d->n_nodes > 0 && d->nodes)) return 0;
	// the per-triangle texture coordinates the shader nodes read
	if(d->tri_uv && (rc = upload(s, d->tri_uv, nt * 6, &out.uv))) return rc;
	if(d->tri_orco && (rc = upload(s, d->tri_orco, nt * 9, &out.orco))) return rc;
	if(s->has_bump)
	{	// the third edge of Triangle::getSurface's dPdU / dPdV (triangle.cc:80-111): c - b, rounded once like e1 and e2 of the record
		std::vector<float> e3(nt * 3);
		for(size_t i = 0; i < nt; ++i) for(int k = 0; k < 3; ++k) e3[3 * i + k] = d->verts[9 * i + 6 + k] - d->verts[9 * i + 3 + k];
		if((rc = upload(s, e3.data(), e3.size(), &out.e3))) return rc;
	}
	return 0;
}

// Faure permutations (the reference ships them as a table, src/common/faure_tables.cc; they are
// the standard construction of Faure 1992 and are regenerated here rather than copied)
static void faure_perm(int b, std::vector<int> &out)
{
	if(b == 2) { out = {0, 1}; return; }
	if(b % 2 == 0)
	{
		std::vector<int> half; faure_perm(b / 2, half);
		out.resize((size_t)b);
		for(int i = 0; i < b / 2; ++i) { out[(size_t)i] = 2 * half[(size_t)i]; out[(size_t)(b / 2 + i)] = 2 * half[(size_t)i] + 1; }
	}
	else
	{
		std::vector<int> prev; faure_perm(b - 1, prev);
		const int m = (b - 1) / 2;
		for(int &v : prev) if(v >= m) ++v;
		out.assign(prev.begin(), prev.begin() + m);
		out.push_back(m);
		out.insert(out.end(), prev.begin() + m, prev.end());
	}
}

static const int kPrimsHost[50] = {1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67,
                                   71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131, 137, 139, 149, 151, 157, 163, 167,
                                   173, 179, 181, 191, 193, 197, 199, 211, 223, 227};

// ---- the steps of yafgpu_scene_create, in its order ---------------------------------------------------------------------------
static int build_tree(yafgpu_scene *s, const yafgpu_scene_desc *d, const AssembledRows &rows)
{
	const int n_tris = (int)rows.n;
	// 0: by size -- the device builder wins from a few ten thousand triangles on (1 M: 0.07 s against 0.33 s)
	bool on_device = d->build_on_device > 0 || (d->build_on_device == 0 && n_tris >= 65536);
	if(const char *e = std::getenv("YAFGPU_BUILD")) on_device = std::strcmp(e, "device") == 0;
	if(on_device)
	{
		std::string err;
		// heavily overlapping geometry can outgrow the builder's arrays: more room, and past that the host builder
		// (same format, same cost model) rather than no tree
		const int brc = build_kdtree_device_retry(rows.verts, n_tris, kDepthCap, s->tree, &err);
		if(brc == -2 || brc == -3) build_kdtree(rows.verts, n_tris, kDepthCap, d->build_threads, s->tree);     // arrays outgrown / no device memory for them
		else if(brc) return fail(-20, err);
	}
	else build_kdtree(rows.verts, n_tris, kDepthCap, d->build_threads, s->tree);
	s->info.build_seconds = s->tree.build_seconds;
	s->info.n_nodes = (uint32_t)s->tree.nodes.size();
	s->info.n_leaf_refs = (uint32_t)s->tree.refs.size();
	s->info.max_depth = (uint32_t)s->tree.max_depth;
	s->info.n_tris = (uint32_t)n_tris;
	return 0;
}

static int upload_tree(yafgpu_scene *s)
{
	DevScene &dv = s->dev;
	int rc = 0;
	if((rc = upload(s, (const uint2 *)s->tree.nodes.data(), s->tree.nodes.size(), &dv.nodes))) return rc;
	// the treelet layout for wf_trace; YAFGPU_TREELET_INLINE=0 sends every non-empty leaf through the escape array (a test aid)
	const char *e = std::getenv("YAFGPU_TREELET_INLINE");
	TreeletLayout tl;
	if(build_treelets(s->tree.nodes, !(e && std::atoi(e) == 0), tl)) return fail(-2, "kd-tree too large for the treelet layout");
	dv.tl_root = tl.root;
	if((rc = upload(s, (const uint4 *)tl.words.data(), tl.words.size() / 4, &dv.treelets))) return rc;
	if((rc = upload(s, (const uint2 *)tl.leaves.data(), tl.leaves.size() / 2, &dv.tl_leaves))) return rc;
	if((rc = upload(s, s->tree.refs.data(), s->tree.refs.size(), &dv.refs))) return rc;
	dv.n_nodes = (uint32_t)s->tree.nodes.size();
	for(int k = 0; k < 3; ++k) { dv.blo[k] = s->tree.bound_lo[k]; dv.bhi[k] = s->tree.bound_hi[k]; }
	return 0;
}

// wf_trace's own copy of the triangle records and of the leaf references (DevScene::tri_walk, refs_walk), in leaf order (kdtree_build.h,
// tri_order).  The rows are on the device (assemble_scene may have made them there), so a kernel makes the copy.  YAFGPU_TRI_ORDER=id keeps
// the copy in id order: the same kernels on the layout the arrays addressed by id have (a comparison aid).
static int upload_walk_copy(yafgpu_scene *s, const AssembledRows &rows)
{
	DevScene &dv = s->dev;
	const uint32_t n = rows.n, n_refs = (uint32_t)s->tree.refs.size();
	std::vector<uint32_t> pos;
	const char *e = std::getenv("YAFGPU_TRI_ORDER");
	if(e && std::strcmp(e, "id") == 0) { pos.resize(n); for(uint32_t t = 0u; t < n; ++t) pos[t] = t; }
	else tri_order(s->tree.refs.data(), s->tree.refs.size(), n, pos);
	DevMem<uint32_t> d_pos;
	float4 *tri_walk = nullptr; uint32_t *refs_walk = nullptr;
	int rc = 0;
	if((rc = temp_upload(d_pos, pos.data(), pos.size())) || (rc = scene_alloc(s, 3 * (size_t)n, &tri_walk)) || (rc = scene_alloc(s, (size_t)n_refs, &refs_walk))) return rc;
	if(n)
	{
		const uint32_t blocks = std::min<uint32_t>((std::max(n, n_refs) + (uint32_t)kBlock - 1u) / (uint32_t)kBlock, 8192u);
		hipLaunchKernelGGL(walk_copy_kernel, dim3(blocks), dim3(kBlock), 0, nullptr, rows.rec, (const uint32_t *)d_pos.p, n, dv.refs, n_refs, tri_walk, refs_walk);
		HIP_OK(hipGetLastError());
		HIP_OK(hipDeviceSynchronize());
	}
	dv.tri_walk = tri_walk; dv.refs_walk = refs_walk;
	return 0;
}

static int upload_lights(yafgpu_scene *s, const yafgpu_scene_desc *d)
{
	s->h_lights.assign(d->lights, d->lights + d->n_lights);
	// a mesh light's Pdf1D row (2 + n + n + 1 floats) follows the triangles of the light-geometry pool, in light order (mesh_light_rows)
	// (the pool's triangles are there for the mesh lights and the portals: without one of them nothing reads, checks or copies them)
	bool with_tris = false;
	for(const yafgpu_light &l : s->h_lights) with_tris = with_tris || l.type == YAFGPU_LIGHT_MESH || l.type == YAFGPU_LIGHT_PORTAL;
	size_t row = with_tris ? (size_t)std::max(d->n_light_tris, 0) * 9 : 0;
	for(yafgpu_light &l : s->h_lights)
		if(l.type == YAFGPU_LIGHT_MESH || l.type == YAFGPU_LIGHT_PORTAL) { l.mesh_row = (int32_t)row; row += 2 * (size_t)l.mesh_count + 3; }
	// a portal's triangle records and normals (16 floats per triangle, read as float4) follow the rows
	row = (row + 3) & ~(size_t)3;
	for(yafgpu_light &l : s->h_lights)
		if(l.type == YAFGPU_LIGHT_PORTAL) { l.mesh_first = row <= (size_t)INT32_MAX ? (int32_t)row : 0; row += 16 * (size_t)l.mesh_count; }
	// the IES lights' tables follow, the whole of the descriptor's pool: a light's ies_first moves by where the pool lands
	s->ies_base = row;
	for(const yafgpu_light &l : s->h_lights) s->has_ies = s->has_ies || l.type == YAFGPU_LIGHT_IES || l.type == YAFGPU_LIGHT_IES_SOFT;
	if(s->has_ies) row += (size_t)d->n_ies_floats;
	for(yafgpu_light &l : s->h_lights)
		if(l.type == YAFGPU_LIGHT_IES || l.type == YAFGPU_LIGHT_IES_SOFT) l.ies_first = row <= (size_t)INT32_MAX ? (int32_t)(s->ies_base + (size_t)l.ies_first) : 0;
	if(row > (size_t)INT32_MAX) return fail(-3, "the light-geometry pool outgrows 2^31 floats");
	s->lgeo_floats = row;
	const int rc = upload(s, s->h_lights.data(), s->h_lights.size(), &s->dev.lights);
	if(rc) return rc;
	s->dev.n_lights = s->n_lights = d->n_lights;
	for(const yafgpu_light &l : s->h_lights) s->light_mask |= 1u << (uint32_t)l.type;
	// a texture background is evaluated per escaping ray by the code that comes with the background light: such a scene asks for a
	// kernel built with that light's bit whether or not the light is there
	if(d->background.kind == YAFGPU_BACKGROUND_TEXTURE) s->light_mask |= 1u << (uint32_t)YAFGPU_LIGHT_BACKGROUND;
	return 0;
}

// image textures: what the shader nodes and a texture background look up
static int upload_textures(yafgpu_scene *s, const yafgpu_scene_desc *d)
{
	DevScene &dv = s->dev;
	std::memset(&dv.tex, 0, sizeof dv.tex);
	if(!((d->n_nodes > 0 && d->nodes) || d->background.kind == YAFGPU_BACKGROUND_TEXTURE)) return 0;
	int rc = 0;
	const float4 *texels = nullptr;
	if((rc = upload(s, d->textures, (size_t)std::max(d->n_textures, 0), &dv.tex.textures))) return rc;
	if((rc = upload(s, (const float4 *)d->texels, (size_t)d->n_texels, &texels))) return rc;
	dv.tex.texels = texels; dv.tex.n_textures = d->n_textures;
	return 0;
}

// shader nodes and the per-triangle texture coordinates they read
static int upload_nodes(yafgpu_scene *s, const yafgpu_scene_desc *d, const AssembledRows &rows)
{
	DevScene &dv = s->dev;
	if(!(d->n_nodes > 0 && d->nodes)) return 0;
	const int rc = upload(s, d->nodes, (size_t)d->n_nodes, &dv.tex.nodes);
	if(rc) return rc;
	dv.tex.tri_uv = rows.uv; dv.tex.tri_orco = rows.orco;
	if(s->has_bump) { dv.tex.tri_e3 = rows.e3; dv.tex.has_bump = 1; }
	return 0;
}

static int upload_qmc_tables(yafgpu_scene *s)
{
	DevScene &dv = s->dev;
	std::vector<int> faure; std::vector<int> foff(50); std::vector<double> invp(50);
	for(int dim = 0; dim < 50; ++dim)
	{
		foff[(size_t)dim] = (int)faure.size();
		std::vector<int> p;
		if(dim < 3) p = {0, 1, 2};      // faure_tables.cc:437: dims 0-2 share the length-3 identity
		else faure_perm(kPrimsHost[dim], p);
		faure.insert(faure.end(), p.begin(), p.end());
		char buf[32];
		std::snprintf(buf, sizeof buf, "%.9f", 1.0 / (double)kPrimsHost[dim]); // scr_halton.h:37-47 prints 9 decimals
		invp[(size_t)dim] = std::strtod(buf, nullptr);
	}
	int rc = 0;
	if((rc = upload(s, faure.data(), faure.size(), &dv.faure))) return rc;
	dv.n_faure = (int)faure.size(); dv.faure_far = dv.faure; dv.faure_near = dv.n_faure;
	if((rc = upload(s, foff.data(), foff.size(), &dv.faure_off))) return rc;
	return upload(s, invp.data(), invp.size(), &dv.inv_prims);
}

// PerspectiveCamera ctor, camera_perspective.cc:42-54: corner table of the polygonal bokeh shapes
static void bokeh_table(yafgpu_camera &cam)
{
	for(float &v : cam.ls) v = 0.f;
	int ns = cam.bokeh_type;
	if(ns < 3 || ns > 6) return;
	float w = (float)((double)cam.bokeh_rotation * 0.01745329251994329576922);
	const float wi = (float)(6.28318530717958647692 / (double)(float)ns);
	ns = (ns + 2) * 2;
	for(int i = 0; i < ns; i += 2)
	{
		cam.ls[i] = host_fsin(w + (float)1.57079632679489661923);     // fCos__
		cam.ls[i + 1] = host_fsin(w);
		w += wi;
	}
}

// BackgroundLight::init: the tables are built where the texture evaluator is, once per scene, from the finished DevScene
static int background_tables(yafgpu_scene *s, const yafgpu_scene_desc *d)
{
	DevScene &dv = s->dev;
	dv.bg.rec = d->background; dv.bg.tab = nullptr; dv.bg.sky = nullptr;
	const bool sky = d->background.kind == YAFGPU_BACKGROUND_GRADIENT || d->background.kind == YAFGPU_BACKGROUND_SUNSKY;
	if(sky) { const int rc = upload(s, &d->sky, 1, &dv.bg.sky); if(rc) return rc; }
	s->has_sky = sky;
	if(d->background.kind == YAFGPU_BACKGROUND_NONE || !d->background.has_ibl) return 0;
	float *tab = nullptr;
	const size_t n_tab = (size_t)(kBgRows + 1) * kBgRowStride;
	if(hipMalloc((void **)&tab, n_tab * sizeof(float)) != hipSuccess) return fail(-100, "no device memory for the background light's tables");
	s->allocs.push_back(tab);
	s->info.device_bytes += n_tab * sizeof(float);
	hipError_t e = hipMemset(tab, 0, n_tab * sizeof(float));
	if(e == hipSuccess)
	{
		hipLaunchKernelGGL(bg_rows_kernel, dim3((uint32_t)kBgRows), dim3(kBlock), 0, nullptr, dv, tab);
		hipLaunchKernelGGL(bg_vdist_kernel, dim3(1), dim3(kBlock), 0, nullptr, tab, sky ? 1 : 0);
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = hipDeviceSynchronize();
	uint32_t bad = 0u;
	if(e == hipSuccess && sky) e = hipMemcpy(&bad, tab + (size_t)kBgRows * kBgRowStride + kBgFlag, sizeof bad, hipMemcpyDeviceToHost);
	if(e != hipSuccess) return fail(-100, std::string("background light tables: ") + hipGetErrorString(e));
	if(bad != 0u)
		return fail(-2, "a sky background with a light needs energy in every latitude row: " + std::to_string(bad & 0xffffu) + " of " + std::to_string(kBgRows) +
		                " rows of the light's tables integrate to nothing or to no finite number" + ((bad >> 16) ? ", and so does their total" : "") +
		                " (Pdf1D would divide by zero; a sun below the horizon or a very low turbidity does this: render the sky without its light)");
	dv.bg.tab = tab;
	return 0;
}

// A portal's triangles have no scene rows, so the triangle records and normals its two leaf functions read are made here, by the kernel that
// makes the scene's rows (assemble_rows: updateIntersectionCachedValues and recNormal), from the corners and the materials of the pool: one
// plain segment per portal, its records to mesh_first, its normals behind them.  Temporaries go when this returns.
static int portal_records(yafgpu_scene *s, const yafgpu_scene_desc *d, float *lgeo)
{
	DevMem<int32_t> p_mat;
	int rc = temp_upload(p_mat, d->light_tri_mat, (size_t)d->n_light_tris);
	if(rc) return rc;
	for(const yafgpu_light &l : s->h_lights)
	{
		if(l.type != YAFGPU_LIGHT_PORTAL) continue;
		yafgpu_segment sg{}; sg.kind = YAFGPU_SEGMENT_PLAIN; sg.first = l.mesh_pool; sg.count = l.mesh_count;
		const uint32_t first[2] = {0u, (uint32_t)l.mesh_count};
		DevMem<yafgpu_segment> d_seg; DevMem<uint32_t> d_first; DevMem<float> d_verts;
		if((rc = temp_upload(d_seg, &sg, 1)) || (rc = temp_upload(d_first, first, 2))) return rc;
		HIP_OK(d_verts.alloc(9 * (size_t)l.mesh_count));
		AssembleArgs a{};
		a.segs = d_seg.p; a.seg_first = d_first.p; a.n_segs = 1; a.n_out = (uint32_t)l.mesh_count;
		a.p_verts = lgeo; a.p_mat = p_mat.p; a.mats = s->dev.mats;
		a.rec = (float4 *)(lgeo + l.mesh_first); a.ng = a.rec + 3 * (size_t)l.mesh_count; a.verts = d_verts.p;
		HIP_OK(assemble_rows(a));
		HIP_OK(hipDeviceSynchronize());
	}
	return 0;
}

// MeshLight::init: the light-geometry pool (the corners of every mesh light's triangles, then a Pdf1D row per light) and each light's area_,
// computed on the device from the corners.  The scene's light records come back with their areas: a light whose mesh has none is refused.
static int mesh_light_rows(yafgpu_scene *s, const yafgpu_scene_desc *d)
{
	DevScene &dv = s->dev;
	dv.lgeo = nullptr;
	const bool portals = (s->light_mask & (1u << (uint32_t)YAFGPU_LIGHT_PORTAL)) != 0u;
	const bool with_tris = (s->light_mask & (1u << (uint32_t)YAFGPU_LIGHT_MESH)) != 0u || portals;
	if(!with_tris && !s->has_ies) return 0;
	float *lgeo = nullptr;
	int rc = scene_alloc(s, s->lgeo_floats, &lgeo);
	if(rc) return rc;
	// the IES lights' tables, as the descriptor has them, behind everything else (upload_lights moved the lights' ies_first there)
	if(s->has_ies) HIP_OK(hipMemcpy(lgeo + s->ies_base, d->ies_tables, (size_t)d->n_ies_floats * sizeof(float), hipMemcpyHostToDevice));
	if(!with_tris) { dv.lgeo = lgeo; return 0; }
	HIP_OK(hipMemcpy(lgeo, d->light_verts, (size_t)d->n_light_tris * 9 * sizeof(float), hipMemcpyHostToDevice));
	hipLaunchKernelGGL(meshlight_rows_kernel, dim3((uint32_t)s->n_lights), dim3(kBlock), 0, nullptr, const_cast<yafgpu_light *>(dv.lights), s->n_lights, lgeo);
	HIP_OK(hipGetLastError());
	if(portals)
	{
		hipLaunchKernelGGL(portallight_rows_kernel, dim3((uint32_t)s->n_lights), dim3(kBlock), 0, nullptr, const_cast<yafgpu_light *>(dv.lights), s->n_lights, lgeo);
		HIP_OK(hipGetLastError());
		if((rc = portal_records(s, d, lgeo))) return rc;
	}
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipMemcpy(s->h_lights.data(), dv.lights, s->h_lights.size() * sizeof(yafgpu_light), hipMemcpyDeviceToHost));
	for(size_t i = 0; i < s->h_lights.size(); ++i)
		if((s->h_lights[i].type == YAFGPU_LIGHT_MESH || s->h_lights[i].type == YAFGPU_LIGHT_PORTAL) && !(s->h_lights[i].area > 0.f && std::isfinite(s->h_lights[i].area)))
			return fail(-3, std::string(s->h_lights[i].type == YAFGPU_LIGHT_PORTAL ? "portal" : "mesh") + " light " + std::to_string(i) + ": the mesh's total area is zero or not finite (Pdf1D would divide by zero)");
	dv.lgeo = lgeo;
	return 0;
}

extern "C" {

const char *yafgpu_last_error(void) { return g_err.c_str(); }
extern "C" void yafgpu_internal_set_error(const char *msg) { g_err = msg ? msg : ""; }

int yafgpu_device_count(void)
{
	int n = 0;
	if(hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}
int yafgpu_set_device(int device) { HIP_OK(hipSetDevice(device)); return 0; }

uint64_t yafgpu_planes_bytes(int32_t width, int32_t height)
{
	return (uint64_t)YAFGPU_FILM_PLANES * (uint64_t)width * (uint64_t)height * YAFGPU_FILM_CHANNELS * sizeof(float);
}

// check, classify, make the rows, build the tree, upload: a scene that fails on the way goes with everything it allocated
int yafgpu_scene_create(const yafgpu_scene_desc *d, yafgpu_scene_t **out)
{
	if(!out) return fail(-1, "null argument");
	int rc = check_desc(d);
	if(rc) return rc;
	std::unique_ptr<yafgpu_scene> owner(new yafgpu_scene());
	yafgpu_scene *s = owner.get();
	classify_materials(s, d);
	// instanced geometry: every row of the scene is made on the device, and the vertices come back for the tree builders
	AssembledRows rows;
	const auto tr = std::chrono::steady_clock::now();
	if(d->inst.n_segments <= 0) host_rows(d, rows);
	else if((rc = assemble_scene(s, d, rows))) return rc;
	const double rows_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tr).count();
	if((rc = build_tree(s, d, rows))) return rc;
	const auto t1 = std::chrono::steady_clock::now();
	DevScene &dv = s->dev;
	if((rc = upload_tree(s)) || (rc = upload_rows(s, d, rows)) || (rc = upload_walk_copy(s, rows))) return rc;
	dv.tri = rows.rec; dv.tri_ng = rows.ng; dv.tri_vn = rows.vn; dv.mats = rows.mats;
	dv.n_tris = (int)rows.n; dv.n_mats = d->n_materials;
	if((rc = upload_lights(s, d)) || (rc = upload_textures(s, d)) || (rc = upload_nodes(s, d, rows)) || (rc = upload_qmc_tables(s))) return rc;
	dv.cam = d->camera;
	bokeh_table(dv.cam);
	s->mats.assign(d->materials, d->materials + d->n_materials);
	if((rc = background_tables(s, d)) || (rc = mesh_light_rows(s, d))) return rc;
	s->info.upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count() + rows_seconds;
	*out = owner.release();
	return 0;
}

void yafgpu_scene_destroy(yafgpu_scene_t *s) { delete s; }      // (device arrays, buffers, streams and events go with their owners)

int yafgpu_scene_info(const yafgpu_scene_t *s, yafgpu_tree_info *info)
{
	if(!s || !info) return fail(-1, "null argument");
	*info = s->info;
	return 0;
}

int yafgpu_scene_get_tree(const yafgpu_scene_t *s, uint32_t *nodes, uint32_t *refs, float bound6[6])
{
	if(!s) return fail(-1, "null argument");
	if(nodes) std::memcpy(nodes, s->tree.nodes.data(), s->tree.nodes.size() * sizeof(KdNode));
	if(refs) std::memcpy(refs, s->tree.refs.data(), s->tree.refs.size() * sizeof(uint32_t));
	if(bound6) for(int k = 0; k < 3; ++k) { bound6[k] = s->tree.bound_lo[k]; bound6[3 + k] = s->tree.bound_hi[k]; }
	return 0;
}

// ---- reconstruction-filter table on the host: ImageFilm ctor + filter functions, src/common/imagefilm.cc:60-121,152-176.
// fExp__/fSin__ are the reference's polynomial approximations (util_math_optimizations.h:116-129,222-244), restated
// for the host so that the table holds the values the reference's film would hold.
static float host_fexp2(float x)
{
	x = std::min(x, 129.00000f);
	x = std::max(x, -126.99999f);
	const int ipart = (int)(x - 0.5f);
	const float p = (x - (float)ipart);
	int bits = (int)((unsigned)(ipart + 127) << 23);
	float expi; std::memcpy(&expi, &bits, 4);
	const float poly = (p * (p * (p * (p * (p * 1.8775767e-3f + 8.9893397e-3f) + 5.5826318e-2f) + 2.4015361e-1f) + 6.9315308e-1f) + 9.9999994e-1f);
	return expi * poly;
}
static float host_fsin(float x)
{
	const double k2Pi = 6.28318530717958647692, kPi = 3.14159265358979323846;
	if((double)x > k2Pi || (double)x < -k2Pi) x -= ((int)(x * (float)0.15915494309189533577)) * (float)k2Pi;
	if((double)x < -kPi) x += (float)k2Pi;
	else if((double)x > kPi) x -= (float)k2Pi;
	x = ((float)1.27323954473516268615 * x) - ((float)0.40528473456935108578 * x * std::fabs(x));
	const float result = 0.225f * (x * std::fabs(x) - x) + x;
	if(result <= -1.0f) return -1.0f;
	if(result >= 1.0f) return 1.0f;
	return result;
}
static float host_filter(int type, float dx, float dy)
{
	switch(type)
	{
		case YAFGPU_FILTER_MITCHELL:
		{
			const float x = 2.f * std::sqrt(dx * dx + dy * dy);
			if(x >= 2.f) return 0.f;
			if(x >= 1.f) return (float)(x * (x * (x * -0.38888889f + 2.0f) - 3.33333333f) + 1.77777778f);
			return (float)(x * x * (1.16666666f * x - 2.0f) + 0.88888889f);
		}
		case YAFGPU_FILTER_GAUSS:
		{
			const float r_2 = dx * dx + dy * dy;
			const float e = host_fexp2((float)1.4426950408889634074 * (float)(-6 * r_2));
			return std::max(0.f, (float)((double)e - 0.00247875));
		}
		case YAFGPU_FILTER_LANCZOS:
		{
			const float x = std::sqrt(dx * dx + dy * dy);
			if(x == 0.f) return 1.f;
			if(-2 < x && x < 2)
			{
				const float a = (float)(3.14159265358979323846 * (double)x), b = (float)(1.57079632679489661923 * (double)x);
				return ((host_fsin(a) * host_fsin(b)) / (a * b));
			}
			return 0.f;
		}
		default: return 1.f;
	}
}
static void host_filter_table(int type, float table[256])
{
	const float scale = 1.f / 16.f;
	for(int y = 0; y < 16; ++y)
		for(int x = 0; x < 16; ++x) table[y * 16 + x] = host_filter(type, (x + .5f) * scale, (y + .5f) * scale);
}

// MIS pairs (shadow parks) of one light estimate of light l: one for a Dirac light, else ceil(samples x multiplier)
// (doLightEstimation, integrator_montecarlo.cc:153)
static_assert(sizeof(yafgpu_light) == 136, "yafgpu_light: the directional / sun / sphere fields overlay the area light's, the record keeps its size");
static int light_pairs(const yafgpu_light &l, float aa_light_sample_multiplier)
{
	return light_type_is_dirac(l.type) ? 1 : (int)std::ceil((float)l.samples * aa_light_sample_multiplier);
}

static int validate(const yafgpu_scene *s, const yafgpu_render_params *rp)
{
	if(rp->width <= 0 || rp->height <= 0 || rp->aa_minsamples <= 0 || rp->tile_size <= 0) return fail(-10, "empty image, sample count or tile size");
	if(rp->xstart < 0 || rp->ystart < 0 || rp->xstart + rp->width > 65535 || rp->ystart + rp->height > 65535) return fail(-10, "render window outside [0, 65535) pixels");
	if(rp->bounces > 12) return fail(-11, "bounces > 12 would use scrHalton dimensions >= 50, which are a global racy LCG in the reference (scr_halton.h:70-73)");
	if(rp->filter_type < YAFGPU_FILTER_BOX || rp->filter_type > YAFGPU_FILTER_LANCZOS) return fail(-12, "unknown filter type");
	if(rp->shard_count < 1 || rp->shard_index < 0 || rp->shard_index >= rp->shard_count) return fail(-13, "bad shard index/count");
	if(rp->integrator != YAFGPU_INTEGRATOR_PATH && rp->integrator != YAFGPU_INTEGRATOR_DIRECT) return fail(-14, "unknown integrator");
	if(rp->path_samples > 8191) return fail(-11, "path_samples > 8191: the device path counts a level's path samples in 13 bits of the control word");
	// the sample index of a light estimate in flight is packed in 12 bits (pack_dlc); validate() runs for every pass, so a
	// light-sample multiplier that grows over the passes of an adaptive render is caught when it gets there
	for(const yafgpu_light &l : s->h_lights)
		if(!light_type_is_dirac(l.type) && std::ceil((float)l.samples * rp->aa_light_sample_multiplier) > 4095.f)
			return fail(-19, "a sampled light (area, sun, sphere, mesh, portal, soft IES or soft spot) with more than 4095 samples per estimate (samples x AA light-sample multiplier): the device path counts them in 12 bits");
	if(rp->do_ao && rp->integrator == YAFGPU_INTEGRATOR_DIRECT)
	{	// ambient occlusion rides the light estimate as the light after the last one (yafgpu_wavefront.h, ao_candidate)
		if(rp->ao_samples < 1) return fail(-19, "ao_samples < 1: the ambient occlusion estimate is divided by its sample count");
		if(rp->ao_samples > 4095) return fail(-19, "ao_samples > 4095: the device path counts the samples of an estimate in 12 bits");
		if(s->h_lights.size() > 254) return fail(-19, "ambient occlusion with more than 254 lights: the device path counts the lights of an estimate, ambient occlusion among them, in 8 bits");
	}
	return 0;
}

// a pipelined pass's counters into the caller's block (accumulate_chunk)
__global__ void add_counters(yafgpu_counters *dst, const yafgpu_counters *src)
{
	const unsigned i = threadIdx.x;
	if(i < sizeof(yafgpu_counters) / sizeof(uint64_t)) ((uint64_t *)dst)[i] += ((const uint64_t *)src)[i];
}

} // extern "C": the pass driver below is internal, and `timed` is a template

// ---- wavefront pass -------------------------------------------------------------------------
static constexpr uint32_t kWfMaxPaths = 32u << 20;   // paths in flight per chunk: 32 Mi x 304 B = 9.5 GiB of parked state

// The environment switches of the render path.  Read at the top of every render call and never kept between
// calls: tests and A/B runs change them between the renders of one process.
struct Switches
{
	uint32_t wf_chunk = kWfMaxPaths;           // YAFGPU_WF_CHUNK: cap on the paths in flight per chunk, at least 256 (tests chunk tiny frames)
	int pass_pipeline = -1, overlap = -1;      // YAFGPU_PASS_PIPELINE, YAFGPU_OVERLAP: 0 / 1 force either; -1: unset, the pass decides (plan_pass)
	bool speculate = true;                     // YAFGPU_SPECULATE=0: the sequential phases (WfArgs::speculate)
	bool multi_pair = true;                    // YAFGPU_MULTI_PAIR=0: one MIS pair per park
	bool hit_cache = true;                     // YAFGPU_HIT_CACHE=0: the final pass of a replay traces its closest hits again
	bool serial_replay = true;                 // YAFGPU_SERIAL_REPLAY=0: per-sample streams instead of the replay
	bool general_shade = false;                // YAFGPU_SHADE_VARIANT=general: the general shading kernel
	bool record_variant = true;                // YAFGPU_RECORD_VARIANT=0: the record pass on the pass's own kernel (A/B)
	bool vertex_lds = true;                    // YAFGPU_VERTEX_LDS=0: every vertex record goes through memory and is stored (WfArgs::vtx_lds, vtx_keep)
	int blocks_per_cu = 8;                     // YAFGPU_BLOCKS_PER_CU: resident workgroups per CU of the persistent kernels (occupancy experiments)
	int trace_grid_cap = 0;                    // YAFGPU_TRACE_GRID_CAP: at most so many workgroups per traversal launch (tests: only with few waves does a batch of 512 * waves * D rays and more start at the largest reservation and drain through every size); 0: no cap
	bool stats = false, verbose = false;       // YAFGPU_STATS, YAFGPU_VERBOSE: set at all
};
static int env_flag(const char *name)      // 1 / 0: set to a number that is / is not zero; -1: unset
{
	const char *e = std::getenv(name);
	return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
}
static Switches read_switches()
{
	Switches sw;
	if(const char *e = std::getenv("YAFGPU_WF_CHUNK")) sw.wf_chunk = std::max(256u, (uint32_t)std::strtoul(e, nullptr, 10));
	sw.pass_pipeline = env_flag("YAFGPU_PASS_PIPELINE");
	sw.overlap = env_flag("YAFGPU_OVERLAP");
	sw.speculate = env_flag("YAFGPU_SPECULATE") != 0;
	sw.multi_pair = env_flag("YAFGPU_MULTI_PAIR") != 0;
	sw.hit_cache = env_flag("YAFGPU_HIT_CACHE") != 0;
	sw.serial_replay = env_flag("YAFGPU_SERIAL_REPLAY") != 0;
	if(const char *e = std::getenv("YAFGPU_SHADE_VARIANT")) sw.general_shade = std::strcmp(e, "general") == 0;
	sw.record_variant = env_flag("YAFGPU_RECORD_VARIANT") != 0;
	sw.vertex_lds = env_flag("YAFGPU_VERTEX_LDS") != 0;
	if(const char *e = std::getenv("YAFGPU_BLOCKS_PER_CU")) sw.blocks_per_cu = std::max(1, std::atoi(e));
	if(const char *e = std::getenv("YAFGPU_TRACE_GRID_CAP")) sw.trace_grid_cap = std::max(0, std::atoi(e));
	sw.stats = std::getenv("YAFGPU_STATS") != nullptr;
	sw.verbose = std::getenv("YAFGPU_VERBOSE") != nullptr;
	return sw;
}

// compute units of the scene's device (s->n_cus), asked once
static int device_cus(yafgpu_scene *s)
{
	if(s->n_cus > 0) return 0;
	int dev = 0; hipDeviceProp_t prop;
	HIP_OK(hipGetDevice(&dev));
	HIP_OK(hipGetDeviceProperties(&prop, dev));
	s->n_cus = prop.multiProcessorCount;
	return 0;
}

static int wf_grid(const void *kernel, int cus, const Switches &sw, bool trace = false)      // trace: a wf_trace instantiation (YAFGPU_TRACE_GRID_CAP applies)
{
	// (the occupancy of a kernel does not change between passes: asked once per kernel)
	static std::mutex mu; static std::map<const void *, int> known;
	int per_cu = 0;
	{
		std::lock_guard<std::mutex> lock(mu);
		auto it = known.find(kernel);
		if(it != known.end()) per_cu = it->second;
		else
		{
			if(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0) != hipSuccess || per_cu < 1) per_cu = 2;
			known[kernel] = per_cu;
		}
	}
	const int grid = cus * std::min(per_cu, sw.blocks_per_cu);
	return (trace && sw.trace_grid_cap > 0) ? std::min(grid, sw.trace_grid_cap) : grid;
}
// workgroups of this process's last closest-hit / any-hit traversal launch, of a render or of a ray batch (yafgpu_trace_schedule: the
// tests read here that YAFGPU_TRACE_GRID_CAP took effect)
static std::atomic<int> g_trace_grid[2] = {{0}, {0}};

// Scene-specialised builds of wf_shade (yafgpu_shade_variant.hip), most specialised first.  A variant serves a scene
// whose material types are a subset of its mask, whose light types are a subset of its light mask (not asked of a record
// pass's program, which has no light code) and which needs recursiveRaytrace only if the variant has it; every
// other scene takes the general kernel of this unit.  YAFGPU_SHADE_VARIANT=general forces the general kernel.
extern "C" {
#define YG_DECLARE_SHADE_VARIANT(name) \
	void yafgpu_shade_##name##_describe(uint32_t *, int *, int *, int *, uint32_t *); const void *yafgpu_shade_##name##_kernel(); \
	int yafgpu_shade_##name##_launch(const void *, size_t, int, hipStream_t);
YG_DECLARE_SHADE_VARIANT(diffuse)
YG_DECLARE_SHADE_VARIANT(glossy)
YG_DECLARE_SHADE_VARIANT(diffuse_mp)
YG_DECLARE_SHADE_VARIANT(glossy_mp)
YG_DECLARE_SHADE_VARIANT(diffuse_rec)
YG_DECLARE_SHADE_VARIANT(glossy_rec)
YG_DECLARE_SHADE_VARIANT(full)
YG_DECLARE_SHADE_VARIANT(blend)
YG_DECLARE_SHADE_VARIANT(meshlight)
YG_DECLARE_SHADE_VARIANT(blend_meshlight)
YG_DECLARE_SHADE_VARIANT(portal)
YG_DECLARE_SHADE_VARIANT(blend_portal)
YG_DECLARE_SHADE_VARIANT(ies)
YG_DECLARE_SHADE_VARIANT(blend_ies)
YG_DECLARE_SHADE_VARIANT(spot)
YG_DECLARE_SHADE_VARIANT(blend_spot)
YG_DECLARE_SHADE_VARIANT(sky)
YG_DECLARE_SHADE_VARIANT(blend_sky)
#undef YG_DECLARE_SHADE_VARIANT
}
struct ShadeVariant
{
	const char *name;
	void (*describe)(uint32_t *, int *, int *, int *, uint32_t *);
	const void *(*kernel)();
	int (*launch)(const void *, size_t, int, hipStream_t);
};
static const ShadeVariant kShadeVariants[] = {
	{"diffuse", yafgpu_shade_diffuse_describe, yafgpu_shade_diffuse_kernel, yafgpu_shade_diffuse_launch},
	{"glossy", yafgpu_shade_glossy_describe, yafgpu_shade_glossy_kernel, yafgpu_shade_glossy_launch},
	// (with a second MIS pair per park, YAFGPU_FEAT_MULTI: for scenes whose light estimates have one to offer)
	{"diffuse_mp", yafgpu_shade_diffuse_mp_describe, yafgpu_shade_diffuse_mp_kernel, yafgpu_shade_diffuse_mp_launch},
	{"glossy_mp", yafgpu_shade_glossy_mp_describe, yafgpu_shade_glossy_mp_kernel, yafgpu_shade_glossy_mp_launch},
	// (the programs of a serial-state replay's record pass: no light estimate, YAFGPU_FEAT_LIGHTS=0)
	{"diffuse_rec", yafgpu_shade_diffuse_rec_describe, yafgpu_shade_diffuse_rec_kernel, yafgpu_shade_diffuse_rec_launch},
	{"glossy_rec", yafgpu_shade_glossy_rec_describe, yafgpu_shade_glossy_rec_kernel, yafgpu_shade_glossy_rec_launch},
	{"full", yafgpu_shade_full_describe, yafgpu_shade_full_kernel, yafgpu_shade_full_launch},      // everything but shader nodes
};
// The general kernel with the blend material's code (YAFGPU_MAT_MASK's bit 8) and every other feature this unit's own wf_shade has: shader
// nodes, the anisotropic lobe, every light type, ambient occlusion, recursion, a second pair per park, and a record pass's program by
// WfArgs::replay as in the general kernel.  Not in the list above: no subset of scenes picks it, a blend in use does.
static const ShadeVariant kBlendVariant = {"blend", yafgpu_shade_blend_describe, yafgpu_shade_blend_kernel, yafgpu_shade_blend_launch};
// The general kernel, and the blend's, with the mesh light's code (YAFGPU_LIGHT_MASK's bit YAFGPU_LIGHT_MESH) and every other feature as well.
// Not in the list either: a mesh light in the scene picks one of them, by whether a blend is in use.
static const ShadeVariant kMeshLightVariant = {"meshlight", yafgpu_shade_meshlight_describe, yafgpu_shade_meshlight_kernel, yafgpu_shade_meshlight_launch};
static const ShadeVariant kBlendMeshLightVariant = {"blend_meshlight", yafgpu_shade_blend_meshlight_describe, yafgpu_shade_blend_meshlight_kernel, yafgpu_shade_blend_meshlight_launch};
// The same two with the portal light's code as well (bits YAFGPU_LIGHT_MESH and YAFGPU_LIGHT_PORTAL): a portal in the scene picks one of them, with or
// without a mesh light beside it.
static const ShadeVariant kPortalVariant = {"portal", yafgpu_shade_portal_describe, yafgpu_shade_portal_kernel, yafgpu_shade_portal_launch};
static const ShadeVariant kBlendPortalVariant = {"blend_portal", yafgpu_shade_blend_portal_describe, yafgpu_shade_blend_portal_kernel, yafgpu_shade_blend_portal_launch};
// And the same two once more with the IES light's two types (bits YAFGPU_LIGHT_IES and YAFGPU_LIGHT_IES_SOFT): every light type's code.  An IES
// light of either kind picks one of them, whatever other lights stand beside it.
static const ShadeVariant kIesVariant = {"ies", yafgpu_shade_ies_describe, yafgpu_shade_ies_kernel, yafgpu_shade_ies_launch};
static const ShadeVariant kBlendIesVariant = {"blend_ies", yafgpu_shade_blend_ies_describe, yafgpu_shade_blend_ies_kernel, yafgpu_shade_blend_ies_launch};
// And once more with the spot light's two types on top (bits YAFGPU_LIGHT_SPOT and YAFGPU_LIGHT_SPOT_SOFT): a spot light of either kind picks one of
// them, before the IES light's, so that a scene with both finds the code of both.
static const ShadeVariant kSpotVariant = {"spot", yafgpu_shade_spot_describe, yafgpu_shade_spot_kernel, yafgpu_shade_spot_launch};
static const ShadeVariant kBlendSpotVariant = {"blend_spot", yafgpu_shade_blend_spot_describe, yafgpu_shade_blend_spot_kernel, yafgpu_shade_blend_spot_launch};
// And once more with the two sky backgrounds' evaluation (YAFGPU_FEAT_SKY) on top of every light type's code: a gradient or a sunsky background
// picks one of them, first, so that a sky beside spot, IES, portal or mesh lights finds the code of all of them; for a record pass too,
// whose escaping rays ask for the sky of their direction.
static const ShadeVariant kSkyVariant = {"sky", yafgpu_shade_sky_describe, yafgpu_shade_sky_kernel, yafgpu_shade_sky_launch};
static const ShadeVariant kBlendSkyVariant = {"blend_sky", yafgpu_shade_blend_sky_describe, yafgpu_shade_blend_sky_kernel, yafgpu_shade_blend_sky_launch};
static const ShadeVariant *pick_shade_variant(const yafgpu_scene *s, const Switches &sw, int frames, bool record_pass, bool want_multi, bool ao)
{
	if(s->has_sky) return s->has_blend ? &kBlendSkyVariant : &kSkyVariant;
	if(s->light_mask & ((1u << (uint32_t)YAFGPU_LIGHT_SPOT) | (1u << (uint32_t)YAFGPU_LIGHT_SPOT_SOFT))) return s->has_blend ? &kBlendSpotVariant : &kSpotVariant;
	if(s->has_ies) return s->has_blend ? &kBlendIesVariant : &kIesVariant;
	if(s->light_mask & (1u << (uint32_t)YAFGPU_LIGHT_PORTAL)) return s->has_blend ? &kBlendPortalVariant : &kPortalVariant;
	// a mesh light: the kernels that have its code, for the same reasons as the blend's below
	if(s->light_mask & (1u << (uint32_t)YAFGPU_LIGHT_MESH)) return s->has_blend ? &kBlendMeshLightVariant : &kMeshLightVariant;
	// a blend material some triangle uses: the one kernel that has its code, whatever the switches say (the general kernel has not) and for
	// the record pass too; a blend nothing uses leaves has_blend clear (yafgpu_scene_create) and the choice below as it was
	if(s->has_blend) return &kBlendVariant;
	if(sw.general_shade || (record_pass && !sw.record_variant)) return nullptr;
	if(ao) return nullptr;                                     // ... and without ambient occlusion (YAFGPU_FEAT_AO)
	const bool needs_recurse = frames > 0 || s->has_volumetric;
	if(s->has_textures || s->has_aniso) return nullptr;        // the variants are built without shader nodes and without the anisotropic lobe
	if(s->dev.bg.rec.kind == YAFGPU_BACKGROUND_TEXTURE) return nullptr;      // ... and without the evaluation of a texture background (a record pass's escaping rays ask for it too)
	for(const ShadeVariant &v : kShadeVariants)
	{
		uint32_t mask = 0u, light_mask = 0u; int recurse = 0, lights = 1, multi = 0;
		v.describe(&mask, &recurse, &lights, &multi, &light_mask);
		if((lights == 0) != record_pass) continue;
		if(lights != 0 && (s->light_mask & ~light_mask) != 0u) continue;
		if(!record_pass && (multi != 0) != want_multi) continue;
		if((s->mat_mask & ~mask) == 0u && (recurse || !needs_recurse)) return &v;
	}
	return nullptr;
}

// Serial-state replay (WfArgs::replay): wanted when the reference's serial state is consumed at all — a roulette test
// can happen (some depth in [1, bounces) lies above russian_roulette_min_bounces) or estimateOneDirectLight has a choice
// (more than one light).  With recursiveRaytrace a sample's events are a tree of integrate() calls, kept per call in the depth-first
// order the reference walks it (up to 255 calls per sample; beyond that the per-sample streams stand in).  The light counter of a SHARDED frame needs every rank's calls per tile (a tile
// starts with the sum over all tiles before it): with an exchange function attached the ranks share them (lc_sharded),
// without one the per-sample ordinals stand in for the counter.
struct ReplayPlan { int frames; bool need_rr, need_lc, replay, replay_lights, lc_sharded; int ev_m; };
static ReplayPlan replay_plan(const yafgpu_scene *s, const yafgpu_render_params &rp, const Switches &sw)
{
	ReplayPlan p{};
	p.frames = ((s->has_specular || s->has_glossy) && rp.raydepth + s->max_add_depth > 0) ? rp.raydepth + s->max_add_depth : 0;
	const bool path = rp.integrator == YAFGPU_INTEGRATOR_PATH;
	p.need_rr = path && rp.bounces - 1 > rp.rr_min_bounces;
	p.need_lc = path && s->n_lights > 1;
	// integrate() calls one camera sample can make (WfArgs::ev_m): without glossy-recursive materials every call sends at most a
	// reflected and a transmitted ray, frames levels deep; with them a call whose trajectory splitting is still 1 also sends 8 glossy
	// trajectories (two rays each through rough glass), whose calls (division >= 8: one trajectory each) send at most 3.  The ordinal has 8 bits.
	{
		long long t = 1, g = 1;
		const long long per_traj = s->has_glossy_two ? 2 : 1;
		for(int k = 0; k < p.frames; ++k) { const long long t2 = s->has_glossy ? 1 + 8 * per_traj * g + 2 * t : 1 + 2 * t; g = 1 + 3 * g; t = std::min<long long>(t2, 1 << 20); }
		p.ev_m = (int)t;
	}
	p.replay = rp.serial_replay != 0 && p.ev_m <= 255 && (p.need_rr || p.need_lc) && sw.serial_replay;
	p.lc_sharded = p.replay && p.need_lc && rp.shard_count > 1 && s->exchange != nullptr;
	p.replay_lights = p.replay && p.need_lc && (rp.shard_count == 1 || p.lc_sharded);
	if(p.replay && !p.need_rr && !p.replay_lights) p.replay = false;
	if(!p.replay) { p.replay_lights = false; p.lc_sharded = false; }
	return p;
}
// The light counter across ranks: every rank contributes the estimateOneDirectLight calls of its own tiles (global tile index,
// count), the exchange function sums the table over the ranks (each entry has one writer; two 16-bit halves as floats, so the sums
// are exact), and every rank takes the same exclusive scan in the reference's tile order on top of the counter so far.  Every rank
// of the render calls this once per pass, with or without tiles of its own.
static int lc_exchange_counts(yafgpu_scene *s, const yafgpu_render_params &rp, const std::vector<std::pair<int, uint32_t>> &own, std::vector<uint32_t> *base_of_tile)
{
	const int ntx = (rp.width + rp.tile_size - 1) / rp.tile_size, nty = (rp.height + rp.tile_size - 1) / rp.tile_size;
	const size_t n = (size_t)ntx * (size_t)nty;
	std::vector<float> h(2 * n, 0.f);
	for(const auto &e : own) { h[2 * (size_t)e.first] = (float)(e.second & 0xffffu); h[2 * (size_t)e.first + 1] = (float)(e.second >> 16); }
	DevMem<float> d;
	HIP_OK(d.alloc(2 * n));
	HIP_OK(hipMemcpy(d, h.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice));
	HIP_OK(hipDeviceSynchronize());
	if(s->exchange(s->exchange_user, d, (uint64_t)(2 * n))) return fail(-31, "the exchange function reported a failure (light counter)");
	HIP_OK(hipMemcpy(h.data(), d, 2 * n * sizeof(float), hipMemcpyDeviceToHost));
	uint32_t run = rp.accumulate ? s->lc_host_counter : 0u;      // zeroed once per render, before its first pass (integrator_tiled.cc:192-194)
	if(base_of_tile) base_of_tile->resize(n);
	for(size_t t = 0; t < n; ++t)
	{
		if(base_of_tile) (*base_of_tile)[t] = run;
		run += (uint32_t)h[2 * t] + ((uint32_t)h[2 * t + 1] << 16);
	}
	s->lc_host_counter = run;
	return 0;
}


// a tile's index among the tiles of the whole frame, row-major (the reference's tile order)
static int tile_global_index(const yafgpu_render_params &rp, const int4 &r)
{
	const int ntx = (rp.width + rp.tile_size - 1) / rp.tile_size;
	return ((r.y - rp.ystart) / rp.tile_size) * ntx + (r.x - rp.xstart) / rp.tile_size;
}

// chunks: runs of pixels whose paths are in flight together (tile_begin, tile_end: with the replay, the tiles it is made of)
struct Chunk { uint32_t pixel_begin, n_pixels, tile_begin, tile_end; };

// What a pass is going to do, decided before anything is enqueued (plan_pass)
struct PassPlan
{
	ReplayPlan rpl{};
	bool stats = false;                        // the counting variant of the traversal kernels
	bool masked = false;                       // a resample mask picks the pixels (adaptive pass)
	std::vector<uint32_t> tile_px;             // pixels of the pass before every tile of the shard
	std::vector<Chunk> chunks;                 // none: the mask picked no pixel of this shard's tiles
	uint32_t spp = 0, cap = 0;                 // cap: paths of the largest chunk
	int frames = 0, frame_recs = 0;            // recursiveRaytrace: a frame of frame_recs records per level a camera hit may recurse to
	uint32_t ev_m = 1, n_ps = 1, n_prob = 1;   // replay: calls per camera sample, path samples per call, roulette probabilities per path sample
	uint32_t hit_k = 0; bool use_hits = false; // the record pass's closest-hit answers per camera sample; kept for the final pass (WfArgs::hit_cache)
	bool want_multi = false, transp = false, overlap = false, piped = false;
	uint32_t vtx_keep = 0xffu;                 // the records 3..10 a park has to store (WfArgs::vtx_keep)
	const ShadeVariant *shade = nullptr, *record = nullptr;      // nullptr: the general kernel / the pass's own kernel
	int iters = 0, iters_record = 0;           // upper bound of kd-tree queries per path = iterations needed (every path advances one query per iteration)
};

// The chunks of a pass.  With the replay a chunk is a run of whole tiles (a tile's stream is walked in one go); without it any run
// of at most max_paths / spp pixels.
static void plan_chunks(size_t n_tiles, uint32_t max_paths, PassPlan &p)
{
	const uint32_t spp = p.spp, n_pixels_total = p.tile_px.back();
	if(p.rpl.replay)
	{
		const uint32_t n_t = (uint32_t)n_tiles;
		for(uint32_t t0 = 0; t0 < n_t;)
		{
			uint32_t t1 = t0 + 1;
			while(t1 < n_t && (uint64_t)(p.tile_px[t1 + 1] - p.tile_px[t0]) * spp <= max_paths) ++t1;
			p.chunks.push_back({p.tile_px[t0], p.tile_px[t1] - p.tile_px[t0], t0, t1});
			t0 = t1;
		}
		return;
	}
	const uint32_t chunk_pixels = std::max(1u, std::min(n_pixels_total, std::max(1u, max_paths / spp)));
	for(uint32_t pb = 0; pb < n_pixels_total; pb += chunk_pixels) p.chunks.push_back({pb, std::min(chunk_pixels, n_pixels_total - pb), 0u, 0u});
}

// Host arithmetic only: nothing is enqueued, allocated or waited for.  (The pixel tables it fills are the scene's because async copies
// read them later.)  The refusals of a pass the device path cannot hold come from here.
static int plan_pass(yafgpu_scene *s, const yafgpu_render_params &rp, const Switches &sw, const ReplayPlan &rpl, bool stats, PassPlan &p)
{
	p.rpl = rpl; p.stats = stats;
	const uint32_t spp = p.spp = (uint32_t)rp.aa_minsamples;
	// per-tile pixel prefix of the shard's tile list
	std::vector<uint32_t> &pp = s->h_pix_prefix;
	pp.assign(1, 0u);
	for(const int4 &r : s->h_tiles) pp.push_back(pp.back() + (uint32_t)(r.z * r.w));
	p.masked = rp.resample_mask != nullptr;
	if(p.masked)
	{	// a resample mask (adaptive pass): the pixels of this shard's tiles that are flagged, in tile order
		std::vector<uint32_t> &listed = s->h_listed;
		listed.clear();
		p.tile_px.assign(1, 0u);
		for(const int4 &r : s->h_tiles)
		{
			for(int y = r.y; y < r.y + r.w; ++y)
				for(int x = r.x; x < r.x + r.z; ++x)
					if(rp.resample_mask[(size_t)(y - rp.ystart) * (size_t)rp.width + (size_t)(x - rp.xstart)]) listed.push_back((uint32_t)x | ((uint32_t)y << 16));
			p.tile_px.push_back((uint32_t)listed.size());
		}
		if(listed.empty()) return 0;      // (no chunks: nothing to render)
	}
	else p.tile_px = pp;
	const uint32_t n_pixels_total = p.tile_px.back();
	{	// Pass pipelining: the pass's path work goes to one of two internal streams with its own buffer set and does NOT wait for what the
		// caller's stream holds (the previous pass, its film combine, a reduce); only the film accumulation is put on the caller's stream, after
		// the path work.  Eligible: one chunk, no serial-state replay (its tables are per scene), no recursion polling, no resample mask (the
		// host reads the film between such passes anyway), no per-kernel profiling.
		// measured (profiles/r03_ab_pipeline.txt): +18 % at an eighth of the metric frame, +10 % at a quarter, +4 % at half, -3 % at the whole
		// frame (two full-size passes only compete) -- on by size, like the two traversal launches side by side
		bool want = s->pass_pipelining < 0 ? (uint64_t)n_pixels_total * spp <= (12ull << 20) : s->pass_pipelining != 0;
		if(sw.pass_pipeline >= 0) want = sw.pass_pipeline != 0;
		p.piped = want && !p.masked && !stats && !s->profiling && !rpl.replay && rpl.frames == 0 && (uint64_t)n_pixels_total * spp <= sw.wf_chunk;
	}
	p.frames = rpl.frames;
	p.frame_recs = s->has_glossy ? (s->has_bump ? 13 : 12) : 5;
	if(p.frames > 7) return fail(-17, "raydepth + additionaldepth > 7 with mirror / transparent / glossy-recursive materials: the device path keeps at most 7 recursion frames per sample");
	const bool path = rp.integrator == YAFGPU_INTEGRATOR_PATH;
	p.n_ps = (uint32_t)std::max(rp.path_samples, 1); p.n_prob = (uint32_t)std::max(rp.bounces - 1, 1);
	p.ev_m = rpl.replay ? (uint32_t)rpl.ev_m : 1u;
	uint32_t max_paths = sw.wf_chunk;
	if(rpl.replay && p.ev_m > 1)
	{	// the event tables grow with the calls a sample can make: keep a chunk's tables within 12 GB
		const uint64_t per_slot = (uint64_t)p.ev_m * p.n_ps * (4 + 4 * p.n_prob + 2) + 4;
		max_paths = (uint32_t)std::min<uint64_t>(max_paths, std::max<uint64_t>((12ull << 30) / per_slot, 4096));
	}
	plan_chunks(s->h_tiles.size(), max_paths, p);
	uint32_t cap_pixels = 1u;
	for(const Chunk &ch : p.chunks) cap_pixels = std::max(cap_pixels, ch.n_pixels);
	if((uint64_t)cap_pixels * spp > (1ull << 27)) return fail(-23, "one tile's samples exceed the 2^27 paths a wavefront chunk can hold: reduce tile_size or the samples per pass");
	p.cap = cap_pixels * spp;
	// transparent shadows only cost anything when a material can be transparent to a shadow ray
	p.transp = rp.transp_shad != 0 && s->has_transparent;
	if(p.transp && rp.shadow_depth > kTsMaxDepth) return fail(-18, "shadowDepth > 8 with transparent shadows: the device path remembers at most 9 filtered triangles per shadow ray");
	if(rpl.replay)
	{	// the record pass's closest-hit answers, one per (call, path sample, segment): kept when a camera sample's fit in 1 KB (the
		// final pass then looks its closest hits up instead of tracing them again); never in a stats pass, whose per-ray traversal
		// counts are the point.  (A pass that replays runs on set 0; wf_hit_key is a 32-bit index.)
		p.hit_k = p.ev_m * p.n_ps * ((uint32_t)std::max(rp.bounces, 1) + 1u);
		const uint32_t set_cap = s->sets[0].cap_for(p.cap, p.frames * p.frame_recs);
		p.use_hits = !stats && (size_t)p.hit_k * sizeof(float4) <= 1024 && (uint64_t)set_cap * p.hit_k < (1ull << 32) && sw.hit_cache;
	}
	// shadow parks (MIS pairs) of the light estimates: all lights of estimateAllDirectLight, the largest of estimateOneDirectLight
	int r_all = 0, r_one = 0;
	for(const yafgpu_light &l : s->h_lights)
	{
		const int r = light_pairs(l, rp.aa_light_sample_multiplier);
		r_all += r; r_one = std::max(r_one, r);
	}
	// ambient occlusion (direct lighting): one more light, a shadow park per sample (two samples per park with WfArgs::multi)
	const bool ao = rp.do_ao != 0 && rp.integrator == YAFGPU_INTEGRATOR_DIRECT;
	if(ao) r_all += std::max(rp.ao_samples, 1);
	// two MIS pairs per park (WfArgs::multi): not with transparent shadows (their filter products are kept per pair), not with recursion frames —
	// and only where a light estimate can have a second pair at all: the kernels that carry it are a little slower on the first
	p.want_multi = !p.transp && p.frames == 0 && sw.multi_pair && r_all > 1;
	// The vertex records a later resume reads (WfArgs::vtx_keep), from the readers in wf_advance.  Everything, whenever a step of a LATER resume
	// rebuilds the vertex: st_start_path for the next path sample (3..6), st_dl_eval / st_beside for the next pair of an estimate that takes
	// several parks (r_all > 1: several lights, or several samples of one), st_recurse* and st_return with recursion frames, st_dl_done's
	// emission under shader nodes, bump or caustic paths (7..10).  Otherwise a later resume reads three words: bsdfs0 (5.w, st_dl_done),
	// integrate()'s w (6.w, the samplers) and the material of the path vertex (7.w, st_dl_done) — those three records are stored, 3, 4, 8, 9 and
	// 10 are not.  What is only known per path is decided there: a park for a shadow pair ALONE (st_beside did not go ahead) stores the whole
	// vertex, for st_extend / st_start_path after the answers, and the pwo a segment that sampled nothing keeps is always stored (vtx_set's keep).
	// A record pass on a light-estimate kernel stores everything too (vtx_flush).
	p.vtx_keep = (sw.vertex_lds && rp.path_samples <= 1 && r_all <= 1 && p.frames == 0 && !s->has_textures && !s->has_bump && !rp.trace_caustics) ? 0x1cu : 0xffu;
	p.shade = pick_shade_variant(s, sw, p.frames, false, p.want_multi, ao);
	if(!p.shade && p.want_multi)
	{	// no kernel with the second pair for these materials: the one without it rather than the general kernel
		p.shade = pick_shade_variant(s, sw, p.frames, false, false, ao);
		if(p.shade) p.want_multi = false;
	}
	// a record pass runs its own, smaller program where one was built for the scene's materials (else the pass's kernel, which branches on WfArgs::replay)
	p.record = rpl.replay ? pick_shade_variant(s, sw, p.frames, true, false, false) : nullptr;
	if(sw.verbose) std::fprintf(stderr, "[yafgpu] shading kernel: %s (materials 0x%x, frames %d), serial replay: %s\n", p.shade ? p.shade->name : "general", s->mat_mask, p.frames,
	                            rpl.replay ? (rpl.replay_lights ? (rpl.need_rr ? "roulette + light counter" : "light counter") : "roulette") : "off");
	p.iters = 1 + r_all;
	if(path) p.iters += std::max(1, rp.path_samples) * ((1 + r_one) + std::max(0, rp.bounces - 1) * (1 + r_one));
	// a record pass asks for closest hits only: the camera ray + per path sample one query per segment
	p.iters_record = 1 + (path ? std::max(1, rp.path_samples) * std::max(1, rp.bounces) : 0);
	// The closest-hit and the any-hit launch of an iteration side by side on two streams (run_program).  On whenever a path parks its next
	// segment beside a vertex's last shadow pair (WfArgs::speculate, the default): the middle phases of a pass then have BOTH queues full,
	// worth +2 % on the whole metric frame (profiles/r03_ab_speculate.txt).  With YAFGPU_SPECULATE=0, by size: chunks under 12 Mi paths,
	// where a persistent launch with a few rays per lane is mostly tail (+5 % at half the metric frame, +8 % at a quarter, +12 % at an
	// eighth, bench.py --emulate-shard).  YAFGPU_OVERLAP=0 / 1 overrides both.  Per-kernel durations overlap in a profiler trace then;
	// the roofline's come from the profiled pass, which keeps one kernel on the GPU at a time either way.
	p.overlap = sw.overlap >= 0 ? sw.overlap != 0 : (sw.speculate || (uint64_t)cap_pixels * spp < (12ull << 20));
	return 0;
}

// One pass on its way: the plan, the buffer set and the streams it runs on
struct PassCtx
{
	yafgpu_scene *s; const PassPlan &p; const Switches &sw; WfSet &w;
	RenderArgs &ra;                      // ra.counters: where the pass's kernels count (a pipelined pass: the set's own block)
	hipStream_t stream, caller;          // the pass's path work; the caller's stream (the same unless the pass is pipelined)
	yafgpu_counters *caller_counters;
	int g_trace_c = 0, g_trace_s = 0, g_shade = 0, g_shade_rec = 0;      // launch grids
	Event ev[2];                         // profiling
	std::vector<std::pair<int, uint32_t>> own_calls;      // sharded light counter: this rank's calls per tile (global tile index, count)
};

// The pipelining prologue: picks the set whose turn it is and orders its stream.  The counters of the pass go to the set's own block.
static int begin_piped_pass(yafgpu_scene *s, hipStream_t caller, bool counters, int &k)
{
	k = s->pipe_next; s->pipe_next ^= 1;
	for(WfSet &o : s->sets) { HIP_OK(o.stream.create()); HIP_OK(o.done.create()); HIP_OK(o.acc.create()); }
	HIP_OK(s->pipe_sync.create());
	WfSet &w = s->sets[k];
	if(counters) HIP_OK(w.counters.reserve(1, w.stream));
	if(!s->pipe_prev)
	{	// the first of a run (or new tile arrays): what the caller's stream holds so far precedes both internal streams, once
		HIP_OK(hipEventRecord(s->pipe_sync, caller));
		for(WfSet &o : s->sets) HIP_OK(hipStreamWaitEvent(o.stream, s->pipe_sync, 0));
	}
	// the set's previous pass has been added to the film (its results and pixel list are free again)
	if(w.acc_set) HIP_OK(hipStreamWaitEvent(w.stream, w.acc, 0));
	if(counters) HIP_OK(hipMemsetAsync(w.counters, 0, sizeof(yafgpu_counters), w.stream));
	return 0;
}

// The set's buffers (and, for a pass that replays, the scene's event tables) large enough for the pass; nothing happens where they are.
static int reserve_workspace(PassCtx &c)
{
	yafgpu_scene *s = c.s; WfSet &w = c.w; const PassPlan &p = c.p; const hipStream_t st = c.stream;
	HIP_OK(w.pix_prefix.reserve(s->h_pix_prefix.size(), st));
	if(w.outgrown(p.cap, p.frames * p.frame_recs)) { w.cap = p.cap; w.frame_recs = p.frames * p.frame_recs; }
	const size_t cap = w.cap;
	HIP_OK(w.state.reserve((size_t)(kWfRecs + w.frame_recs) * cap, st));
	HIP_OK(w.results.reserve(cap, st));
	// two queue sets, each: closest (cap), shadow rays (4*cap: up to two MIS pairs per park), resume (cap)
	HIP_OK(w.queues.reserve(12 * cap, st));
	HIP_OK(w.verdict.reserve((4 * cap + 31) / 32 + 16, st));      // one bit per shadow ray (+ 64 bytes)
	HIP_OK(w.pix_xy.reserve(cap, st));          // pixels of a chunk <= paths of a chunk
	HIP_OK(w.counts.reserve(64, st));           // two sets of 32 (in / out)
	if(p.transp) HIP_OK(w.filt.reserve(2 * cap, st));
	if(p.rpl.replay)
	{	// event tables of the record pass, per path sample
		const size_t ents = cap * p.ev_m * p.n_ps;
		HIP_OK(s->rp_flags.reserve(ents, st));
		HIP_OK(s->rp_p.reserve(ents * p.n_prob, st));
		HIP_OK(s->rp_kill.reserve(ents, st));
		HIP_OK(s->rp_calls.reserve(ents, st));
		HIP_OK(s->rp_base.reserve(cap, st));
		if(p.use_hits) HIP_OK(s->rp_hits.reserve(cap * p.hit_k, st));
		HIP_OK(s->rp_counter.reserve(1, st));
	}
	return 0;
}

// Every chunk's tiles as segments — first pixel of each (chunk-local) and the seed of its Random:
// rand() + offset * (resx * tile.y + tile.x) + 123 (integrator_tiled.cc:319), offset = pass offset + base sampling
// offset (:203,263).  One table for the whole pass, uploaded once: chunk k reads its slice [seg_off[k], ...).
static int upload_segments(PassCtx &c)
{
	yafgpu_scene *s = c.s; const PassPlan &p = c.p; const yafgpu_render_params &rp = c.ra.rp;
	HIP_OK(hipStreamSynchronize(c.stream));        // the previous pass's upload of the table has been read
	s->h_seg_begin.clear(); s->h_seg_seed.clear();
	const uint32_t offset = rp.pass_offset + rp.base_sampling_offset;
	for(const Chunk &ch : p.chunks)
	{
		for(uint32_t t = ch.tile_begin; t <= ch.tile_end; ++t) s->h_seg_begin.push_back(p.tile_px[t] - ch.pixel_begin);
		for(uint32_t t = ch.tile_begin; t < ch.tile_end; ++t)
		{
			const int4 &r = s->h_tiles[t];
			const uint32_t rnd = rp.tile_rand ? (uint32_t)rp.tile_rand[tile_global_index(rp, r)] : 0u;
			s->h_seg_seed.push_back(rnd + offset * ((uint32_t)s->dev.cam.resx * (uint32_t)r.y + (uint32_t)r.x) + 123u);
		}
		s->h_seg_seed.push_back(0u);           // keeps the two tables aligned (n + 1 entries per chunk)
	}
	if(c.sw.verbose)
	{
		std::fprintf(stderr, "[yafgpu] replay pass_offset %u accumulate %d spp %u: seeds", rp.pass_offset, rp.accumulate, p.spp);
		for(size_t k = 0; k < std::min<size_t>(s->h_seg_seed.size(), 6); ++k) std::fprintf(stderr, " %u", s->h_seg_seed[k]);
		std::fprintf(stderr, " ... entries/tile");
		for(size_t k = 0; k + 1 < std::min<size_t>(s->h_seg_begin.size(), 7); ++k) std::fprintf(stderr, " %u", s->h_seg_begin[k + 1] - s->h_seg_begin[k]);
		std::fprintf(stderr, "\n");
	}
	const size_t segs = s->h_seg_begin.size();
	HIP_OK(s->rp_seg_begin.reserve(segs, c.stream));
	HIP_OK(s->rp_seg_seed.reserve(segs, c.stream));
	HIP_OK(s->rp_seg_total.reserve(segs, c.stream));
	HIP_OK(s->rp_seg_base.reserve(segs, c.stream));
	HIP_OK(hipMemcpyAsync(s->rp_seg_begin, s->h_seg_begin.data(), segs * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
	HIP_OK(hipMemcpyAsync(s->rp_seg_seed, s->h_seg_seed.data(), segs * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
	// correlative_sample_number_ is zeroed once per render, before its first pass (integrator_tiled.cc:192-194)
	if(!rp.accumulate) HIP_OK(hipMemsetAsync(s->rp_counter, 0, sizeof(uint32_t), c.stream));
	return 0;
}

// The one place that records profiling events: a launch on the pass's stream and, under profiling, its duration into `slot`
// (yafgpu_get_profile: trace closest, trace shadow, shade, other).
template<typename F> static int timed(PassCtx &c, int slot, F &&launch)
{
	yafgpu_scene *s = c.s;
	if(s->profiling) HIP_OK(hipEventRecord(c.ev[0], c.stream));
	launch();
	HIP_OK(hipGetLastError());
	if(s->profiling)
	{
		HIP_OK(hipEventRecord(c.ev[1], c.stream));
		HIP_OK(hipEventSynchronize(c.ev[1]));
		float ms = 0.f; HIP_OK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
		s->prof_ms[slot] += ms; s->prof_launches[slot] += 1;
	}
	return 0;
}

// One run of the path program over a chunk: generate, then iterations of {closest-hit, any-hit, shade} until
// every path has ended.  Without recursion the number of queries per path is bounded a priori (n_iters) and the
// loop never asks the device anything.  With recursiveRaytrace a sample may visit up to 2^raydepth levels, so past
// that bound the loop runs on while any queue is non-empty (one 20-byte read-back per iteration).
static int run_program(PassCtx &c, WfArgs &a, int n_iters, bool record)
{
	yafgpu_scene *s = c.s; WfSet &w = c.w; const PassPlan &p = c.p; const hipStream_t stream = c.stream;
	const int cus = s->n_cus;
	const size_t cp = w.cap;
	uint32_t *const qset[2][3] = {{w.queues, w.queues + cp, w.queues + 5 * cp},
	                              {w.queues + 6 * cp, w.queues + 7 * cp, w.queues + 11 * cp}};   // closest, shadow rays (4*cap), resume
	uint32_t *const cnt[2] = {w.counts, w.counts + 32};
	int rc;
	a.cnt_in = cnt[0]; a.cnt_out = cnt[1];
	a.q_closest_in = nullptr; a.q_shadow_in = qset[0][1]; a.q_resume_in = qset[0][2];
	a.q_closest_out = qset[1][0]; a.q_shadow_out = qset[1][1]; a.q_resume_out = qset[1][2];
	const uint32_t g_gen = std::min<uint32_t>((a.n_paths + kBlock - 1) / kBlock, (uint32_t)cus * 8u);
	{	// A camera whose samples may carry no ray (the circular angular camera) has wf_generate list the live ones in the first iteration's
		// closest-hit queue, counted from zero; every other camera keeps the identity queue and a count of n_paths.  The perspective and
		// architect cameras run the kernel's instance without the other two types' code.
		const int cam_type = a.ra.sc.cam.type;
		const bool panoramic = cam_type == YAFGPU_CAMERA_ANGULAR || cam_type == YAFGPU_CAMERA_EQUIRECTANGULAR;
		const bool may_die = cam_type == YAFGPU_CAMERA_ANGULAR && a.ra.sc.cam.circular != 0;
		WfArgs g = a;
		g.q_closest_out = may_die ? qset[0][0] : nullptr;
		if(may_die)
		{
			HIP_OK(hipMemsetAsync(a.cnt_in, 0, 8 * sizeof(uint32_t), stream));
			a.q_closest_in = qset[0][0];
		}
		if((rc = timed(c, 3, [&] {
			if(panoramic) hipLaunchKernelGGL(wf_generate<true>, dim3(g_gen), dim3(kBlock), 0, stream, g);
			else hipLaunchKernelGGL(wf_generate<false>, dim3(g_gen), dim3(kBlock), 0, stream, g); }))) return rc;
	}
	int cur = 0;
	const int iter_cap = n_iters * (p.frames > 0 ? (1 << (p.frames + 1)) : 1) * (s->has_glossy ? (s->has_glossy_two ? 32 : 16) : 1);      // (a safety net: the loop ends when the queues are empty)
	// the record pass answered the final pass's closest-hit queries already: wf_shade reads them from its cache where it would read the traversal's answers
	const bool trace_closest = record || a.replay != 2 || a.hit_cache == nullptr;
	for(int it = 0; it < iter_cap; ++it)
	{
		if(p.frames > 0 && it >= n_iters)
		{
			uint32_t pending[5];
			HIP_OK(hipMemcpyAsync(pending, a.cnt_in, sizeof pending, hipMemcpyDeviceToHost, stream));
			HIP_OK(hipStreamSynchronize(stream));
			if(pending[0] == 0u && pending[1] == 0u && pending[4] == 0u) break;
		}
		else if(p.frames == 0 && it >= n_iters) break;
		HIP_OK(hipMemsetAsync(a.cnt_out, 0, 8 * sizeof(uint32_t), stream));
		// The two traversal launches of an iteration are independent (each drains its own queue, writes its own
		// answers), and a persistent kernel's tail leaves CUs idle: outside profiling the any-hit launch goes to a
		// side stream so that its waves fill the closest-hit launch's tail (and vice versa).
		const bool fork = p.overlap && it > 0 && !s->profiling && !record;
		const hipStream_t any_stream = fork ? (hipStream_t)w.side : stream;
		if(fork)
		{	// fork point: everything enqueued so far (the previous shade, the counter reset) precedes both launches
			HIP_OK(hipEventRecord(w.fork, stream));
			HIP_OK(hipStreamWaitEvent(w.side, w.fork, 0));
		}
		if(trace_closest && (rc = timed(c, 0, [&] {
			if(p.stats) hipLaunchKernelGGL((wf_trace<false, true>), dim3(c.g_trace_c), dim3(kBlock), 0, stream, a);
			else hipLaunchKernelGGL((wf_trace<false, false>), dim3(c.g_trace_c), dim3(kBlock), 0, stream, a); }))) return rc;
		if(it > 0 && !record)      // (a record pass has no shadow rays)
		{
			HIP_OK(hipMemsetAsync(w.verdict, 0, ((size_t)4 * a.n_paths + 31) / 32 * sizeof(uint32_t), any_stream));     // occluded rays set their bit
			if((rc = timed(c, 1, [&] {
				if(p.transp && c.s->has_blend) hipLaunchKernelGGL((wf_trace_ts<true>), dim3(cus * 8), dim3(kBlock), 0, any_stream, a);
				else if(p.transp) hipLaunchKernelGGL((wf_trace_ts<false>), dim3(cus * 8), dim3(kBlock), 0, any_stream, a);
				else if(p.stats) hipLaunchKernelGGL((wf_trace<true, true>), dim3(c.g_trace_s), dim3(kBlock), 0, any_stream, a);
				else hipLaunchKernelGGL((wf_trace<true, false>), dim3(c.g_trace_s), dim3(kBlock), 0, any_stream, a); }))) return rc;
		}
		if(fork)
		{
			HIP_OK(hipEventRecord(w.join, w.side));
			HIP_OK(hipStreamWaitEvent(stream, w.join, 0));
		}
		int variant_rc = 0;
		if((rc = timed(c, 2, [&] {
			if(record && p.record) variant_rc = p.record->launch(&a, sizeof a, c.g_shade_rec, stream);
			else if(p.shade) variant_rc = p.shade->launch(&a, sizeof a, c.g_shade, stream);
			else hipLaunchKernelGGL(wf_shade, dim3(c.g_shade), dim3(kBlock), 0, stream, a); }))) return rc;
		if(variant_rc) return fail(-21, "shading kernel variant and main unit disagree on the argument layout");
		// swap queues: what shade produced is the next iteration's input
		cur ^= 1;
		a.cnt_in = cnt[cur]; a.cnt_out = cnt[cur ^ 1];
		a.q_closest_in = qset[cur][0]; a.q_shadow_in = qset[cur][1]; a.q_resume_in = qset[cur][2];
		a.q_closest_out = qset[cur ^ 1][0]; a.q_shadow_out = qset[cur ^ 1][1]; a.q_resume_out = qset[cur ^ 1][2];
	}
	return 0;
}

// The serial-state replay of a chunk, up to the final pass's program: the record pass, then the walk of the tiles' streams.
// phase 0: all of it.  A sharded light counter splits it: phase 1 = the record pass, the tiles' roulette walk and their call counts
// (read back into c.own_calls); phase 2 = the rest, from the bases the ranks' exchange gave (a pass of one chunk keeps its events
// from phase 1, one of several records them again).
static int replay_chunk(PassCtx &c, const Chunk &ch, WfArgs &a, size_t seg_off, int phase)
{
	yafgpu_scene *s = c.s; const PassPlan &p = c.p; const yafgpu_render_params &rp = c.ra.rp; const hipStream_t stream = c.stream;
	int rc;
	const bool have_events = phase == 2 && p.chunks.size() == 1;
	if(!have_events)
	{	// record pass: the paths alone (no light estimates, no roulette kills), rays not counted
		a.replay = 1;
		yafgpu_counters *const keep = a.ra.counters;
		a.ra.counters = nullptr;
		HIP_OK(hipMemsetAsync(s->rp_flags, 0, (size_t)a.n_paths * p.ev_m * p.n_ps * sizeof(uint32_t), stream));
		if((rc = run_program(c, a, p.iters_record, true))) return rc;
		a.ra.counters = keep;
	}
	const uint32_t n_seg = ch.tile_end - ch.tile_begin;
	ReplayArgs r{};
	r.seg_begin = s->rp_seg_begin + seg_off; r.seg_seed = s->rp_seg_seed + seg_off; r.n_seg = n_seg; r.spp = p.spp; r.n_paths = p.ev_m * p.n_ps; r.n_prob = p.n_prob;
	r.bounces = (uint32_t)std::max(rp.bounces, 1);
	r.ev_flags = s->rp_flags; r.ev_p = s->rp_p; r.ev_kill = s->rp_kill; r.ev_calls = s->rp_calls; r.lc_base = s->rp_base;
	r.seg_total = s->rp_seg_total + seg_off; r.lc_counter = s->rp_counter;
	r.seg_base_in = phase == 2 ? s->rp_seg_base + seg_off : nullptr;
	if((rc = timed(c, 3, [&] {
		if(!have_events) hipLaunchKernelGGL(wf_replay_tiles, dim3(n_seg), dim3(kWave), 0, stream, r);
		if(phase == 0) hipLaunchKernelGGL(wf_replay_bases, dim3(1), dim3(1), 0, stream, r);
		if(phase != 1) hipLaunchKernelGGL(wf_replay_samples, dim3(n_seg), dim3(kWave), 0, stream, r); }))) return rc;
	if(phase == 1)
	{	// this chunk's calls per tile, by global tile index
		std::vector<uint32_t> totals(n_seg);
		HIP_OK(hipMemcpyAsync(totals.data(), s->rp_seg_total + seg_off, n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		for(uint32_t k = 0; k < n_seg; ++k) c.own_calls.emplace_back(tile_global_index(rp, s->h_tiles[ch.tile_begin + k]), totals[k]);
		return 0;
	}
	if(c.sw.verbose)
	{
		uint32_t cnt_now = 0;
		HIP_OK(hipMemcpyAsync(&cnt_now, s->rp_counter, sizeof cnt_now, hipMemcpyDeviceToHost, stream));
		HIP_OK(hipStreamSynchronize(stream));
		std::fprintf(stderr, "[yafgpu] replay chunk of %u tiles: light counter now %u\n", n_seg, cnt_now);
	}
	a.replay = 2;
	return 0;
}

// The chunk's results into the film.  A pipelined pass adds them on the caller's stream, after its path work and (by that stream's
// order) after the previous pass's film, and its counters to the caller's.
static int accumulate_chunk(PassCtx &c, const WfArgs &a)
{
	WfSet &w = c.w;
	const uint32_t g_acc = std::min<uint32_t>((a.n_pixels + kBlock - 1) / kBlock, (uint32_t)c.s->n_cus * 8u);
	if(!c.p.piped) return timed(c, 3, [&] { hipLaunchKernelGGL(wf_accumulate, dim3(g_acc), dim3(kBlock), 0, c.stream, a); });
	HIP_OK(hipEventRecord(w.done, c.stream));
	HIP_OK(hipStreamWaitEvent(c.caller, w.done, 0));
	WfArgs acc = a;
	acc.ra.counters = c.caller_counters;
	hipLaunchKernelGGL(wf_accumulate, dim3(g_acc), dim3(kBlock), 0, c.caller, acc);
	if(c.caller_counters) hipLaunchKernelGGL(add_counters, dim3(1), dim3(64), 0, c.caller, c.caller_counters, (const yafgpu_counters *)w.counters);
	HIP_OK(hipGetLastError());
	HIP_OK(hipEventRecord(w.acc, c.caller));
	w.acc_set = true;
	return 0;
}

// One chunk of the pass: its arguments, the replay where there is one, the path program, the film.  seg_off: where the chunk's
// slice of the segment tables begins (advanced past it).
static int process_chunk(PassCtx &c, const Chunk &ch, size_t &seg_off, int phase)
{
	yafgpu_scene *s = c.s; WfSet &w = c.w; const PassPlan &p = c.p;
	if(s->aborted()) return fail(-30, "aborted");
	WfArgs a{};
	a.ra = c.ra;
	a.state = w.state; a.cap = w.cap; a.results = w.results; a.frames = p.frames; a.frame_recs = p.frame_recs; a.has_glossy = s->has_glossy ? 1 : 0;
	a.pixel_begin = ch.pixel_begin; a.n_pixels = ch.n_pixels; a.n_paths = a.n_pixels * p.spp;
	a.pix_prefix = w.pix_prefix; a.pix_xy = w.pix_xy; a.pix_listed = p.masked ? 1 : 0;
	if(p.masked) HIP_OK(hipMemcpyAsync(w.pix_xy, s->h_listed.data() + ch.pixel_begin, (size_t)a.n_pixels * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
	a.ev_flags = s->rp_flags; a.ev_p = s->rp_p; a.ev_kill = s->rp_kill; a.ev_calls = s->rp_calls; a.lc_base = s->rp_base;
	a.replay_lights = p.rpl.replay_lights ? 1 : 0; a.ev_m = (int)p.ev_m;
	a.multi = p.want_multi ? 1 : 0;
	a.speculate = c.sw.speculate ? 1 : 0;
	a.vtx_lds = c.sw.vertex_lds ? 1 : 0; a.vtx_keep = p.vtx_keep;
	a.hit_cache = p.use_hits ? (float4 *)s->rp_hits : nullptr; a.hit_k = (int)p.hit_k;
	a.verdict = w.verdict; a.shadow_filt = p.transp ? (float4 *)w.filt : nullptr;
	int rc;
	if(p.rpl.replay)
	{
		rc = replay_chunk(c, ch, a, seg_off, phase);
		seg_off += ch.tile_end - ch.tile_begin + 1;
		if(rc || phase == 1) return rc;
	}
	if((rc = run_program(c, a, p.iters, false))) return rc;
	return accumulate_chunk(c, a);
}

static int render_wavefront(yafgpu_scene *s, RenderArgs &ra, const Switches &sw, const ReplayPlan &rpl, hipStream_t caller, bool stats)
{
	const yafgpu_render_params &rp = ra.rp;
	if(rp.resample_mask) HIP_OK(hipStreamSynchronize(caller));      // the previous pass's uploads of the pixel list (s->h_listed) have been read
	PassPlan p;
	int rc = plan_pass(s, rp, sw, rpl, stats, p);
	if(rc) return rc;
	if(p.chunks.empty()) return rpl.lc_sharded ? lc_exchange_counts(s, rp, {}, nullptr) : 0;      // (the other ranks wait for this one's counts)
	int k = 0;      // passes that are not pipelined: set 0, on the caller's stream
	if(p.piped && (rc = begin_piped_pass(s, caller, ra.counters != nullptr, k))) return rc;
	s->pipe_prev = p.piped;
	WfSet &w = s->sets[k];
	PassCtx c{s, p, sw, w, ra, p.piped ? (hipStream_t)w.stream : caller, caller, ra.counters};
	if(p.piped && ra.counters) ra.counters = w.counters;
	if((rc = reserve_workspace(c))) return rc;
	// on the pass's stream: kernels of the previous pass may still be reading the table (a null-stream copy does not order against a
	// non-blocking stream); the source is pageable, so the call returns once it has been staged
	HIP_OK(hipMemcpyAsync(w.pix_prefix, s->h_pix_prefix.data(), s->h_pix_prefix.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
	if(rpl.replay && (rc = upload_segments(c))) return rc;
	if((rc = device_cus(s))) return rc;
	c.g_trace_c = stats ? wf_grid((const void *)wf_trace<false, true>, s->n_cus, sw, true) : wf_grid((const void *)wf_trace<false, false>, s->n_cus, sw, true);
	c.g_trace_s = stats ? wf_grid((const void *)wf_trace<true, true>, s->n_cus, sw, true) : wf_grid((const void *)wf_trace<true, false>, s->n_cus, sw, true);
	g_trace_grid[0] = c.g_trace_c; g_trace_grid[1] = c.g_trace_s;
	c.g_shade = wf_grid(p.shade ? p.shade->kernel() : (const void *)wf_shade, s->n_cus, sw);
	c.g_shade_rec = p.record ? wf_grid(p.record->kernel(), s->n_cus, sw) : c.g_shade;
	if(p.overlap) { HIP_OK(w.side.create()); HIP_OK(w.fork.create()); HIP_OK(w.join.create()); }
	if(s->profiling)
	{
		for(Event &e : c.ev) HIP_OK(e.create(hipEventDefault));
		for(int i = 0; i < 4; ++i) { s->prof_ms[i] = 0; s->prof_launches[i] = 0; }
	}
	if(rpl.lc_sharded)
	{	// phase 1 for every chunk, then the ranks exchange the counts
		size_t seg_off = 0;
		for(const Chunk &ch : p.chunks) if((rc = process_chunk(c, ch, seg_off, 1))) return rc;
		std::vector<uint32_t> base_of_tile;
		if((rc = lc_exchange_counts(s, rp, c.own_calls, &base_of_tile))) return rc;
		// the bases in the layout of the segment tables (n + 1 entries per chunk)
		s->h_seg_base.clear();
		for(const Chunk &ch : p.chunks)
		{
			for(uint32_t t = ch.tile_begin; t < ch.tile_end; ++t) s->h_seg_base.push_back(base_of_tile[(size_t)tile_global_index(rp, s->h_tiles[t])]);
			s->h_seg_base.push_back(0u);
		}
		HIP_OK(hipMemcpyAsync(s->rp_seg_base, s->h_seg_base.data(), s->h_seg_base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.stream));
	}
	size_t seg_off = 0;
	for(const Chunk &ch : p.chunks) if((rc = process_chunk(c, ch, seg_off, rpl.lc_sharded ? 2 : 0))) return rc;
	return 0;
}

extern "C" {      // the ABI again

int yafgpu_render_tiles(yafgpu_scene_t *s, const yafgpu_render_params *rp, float *d_planes, yafgpu_counters *d_counters, void *stream_)
{
	if(!s || !rp || !d_planes) return fail(-1, "null argument");
	int rc = validate(s, rp);
	if(rc) return rc;
	hipStream_t stream = (hipStream_t)stream_;
	const Switches sw = read_switches();
	const ReplayPlan rpl = replay_plan(s, *rp, sw);
	RenderArgs ra{};
	ra.sc = s->dev;
	ra.rp = *rp;
	ra.shadow_bias = rp->shadow_bias_auto ? kShadowBias : rp->shadow_bias;     // scene.cc:825
	ra.ray_min_dist = rp->min_raydist_auto ? kMinRayDist : rp->min_raydist;    // scene.cc:826
	{	// ImageFilm ctor, imagefilm.cc:127,152-176: half-width, per-type widening, clamp to [0.501, 4], 16x16 table
		float fw = (float)((double)rp->aa_pixelwidth * 0.5);
		if(rp->filter_type == YAFGPU_FILTER_MITCHELL) fw *= 2.6f;
		else if(rp->filter_type == YAFGPU_FILTER_GAUSS) fw *= 2.f;
		ra.filterw = std::min(std::max(0.501f, fw), 0.5f * 8.f);
		ra.table_scale = (float)(0.9999 * 16 / (double)ra.filterw);
		ra.wide_filter = (rp->filter_type != YAFGPU_FILTER_BOX || ra.filterw > 0.501f) ? 1 : 0;
		ra.filter_table = nullptr;
		if(ra.wide_filter)
		{
			float table[256];
			host_filter_table(rp->filter_type, table);
			HIP_OK(s->d_filter_table.reserve(256, stream));
			HIP_OK(hipMemcpyAsync(s->d_filter_table, table, sizeof table, hipMemcpyHostToDevice, stream));
			ra.filter_table = s->d_filter_table;
		}
	}
	// tiles of this shard, row-major (ImageSplitter linear order, imagesplitter.cc:30-60)
	const int key[7] = {rp->width, rp->height, rp->xstart, rp->ystart, rp->tile_size, rp->shard_index, rp->shard_count};
	const bool same = std::memcmp(key, s->tile_key, sizeof key) == 0;
	if(!same)
	{
		const int ntx = (rp->width + rp->tile_size - 1) / rp->tile_size, nty = (rp->height + rp->tile_size - 1) / rp->tile_size;
		std::vector<int4> &tiles = s->h_tiles;
		tiles.clear();
		for(int t = 0; t < ntx * nty; ++t)
		{
			if(t % rp->shard_count != rp->shard_index) continue;
			const int tx = t % ntx, ty = t / ntx;
			int4 r;
			r.x = rp->xstart + tx * rp->tile_size; r.y = rp->ystart + ty * rp->tile_size;
			r.z = std::min(rp->tile_size, rp->xstart + rp->width - r.x); r.w = std::min(rp->tile_size, rp->ystart + rp->height - r.y);
			tiles.push_back(r);
		}
	}
	ra.n_tiles = (int)s->h_tiles.size();
	if(!rp->accumulate) HIP_OK(hipMemsetAsync(d_planes, 0, yafgpu_planes_bytes(rp->width, rp->height), stream));
	if(ra.n_tiles == 0)      // a rank without tiles still owes the others its (empty) share of the light-counter exchange
		return rpl.lc_sharded ? lc_exchange_counts(s, *rp, {}, nullptr) : 0;
	if(!same)
	{
		HIP_OK(s->d_tiles.reserve(s->h_tiles.size(), stream));      // (the previous pass may still read the old array)
		HIP_OK(hipMemcpyAsync(s->d_tiles, s->h_tiles.data(), s->h_tiles.size() * sizeof(int4), hipMemcpyHostToDevice, stream));
		std::memcpy(s->tile_key, key, sizeof key);
		s->pipe_prev = false;      // (pipelined passes: the new tile arrays precede the internal streams' next launches)
	}
	ra.tile_rect = s->d_tiles;
	ra.planes = d_planes;
	ra.counters = d_counters;
	return render_wavefront(s, ra, sw, rpl, stream, d_counters != nullptr && sw.stats);
}

int yafgpu_film_combine(const float *d_planes, float *d_film, int32_t width, int32_t height, void *stream_)
{
	if(!d_planes || !d_film || width <= 0 || height <= 0) return fail(-1, "bad argument");
	const size_t n = (size_t)width * (size_t)height;
	const uint32_t grid = (uint32_t)std::min<size_t>((n + kBlock - 1) / kBlock, 2048);
	hipLaunchKernelGGL(combine_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream_, d_planes, d_film, width, height);
	HIP_OK(hipGetLastError());
	return 0;
}

// planes, combined film and counters of a w x h frame, owned by the scene and reused while the size stays
static int render_targets(yafgpu_scene *s, int w, int h, float **planes, float **film, yafgpu_counters **cnt)
{
	HIP_OK(s->rt_planes.reserve(yafgpu_planes_bytes(w, h) / sizeof(float), nullptr));
	HIP_OK(s->rt_film.reserve((size_t)w * (size_t)h * YAFGPU_FILM_CHANNELS, nullptr));
	HIP_OK(s->rt_cnt.reserve(1, nullptr));
	*planes = s->rt_planes; *film = s->rt_film; *cnt = s->rt_cnt;
	return 0;
}

// The output stage on the film a render left in the scene's render targets: converted where it lies, only the packed image comes down
int yafgpu_scene_film_to_image(yafgpu_scene_t *s, const yafgpu_image_desc *desc, void *h_image)
{
	if(!s || !desc || !h_image) return fail(-1, "film to image: null argument");
	if(s->rt_film_w <= 0 || !s->rt_film.p) return fail(-13, "film to image: the scene holds no finished film (render first)");
	if(desc->width != s->rt_film_w || desc->height != s->rt_film_h)
		return fail(-13, "film to image: the scene's film is " + std::to_string(s->rt_film_w) + " x " + std::to_string(s->rt_film_h) + ", not " +
		                 std::to_string(desc->width) + " x " + std::to_string(desc->height));
	const uint64_t bytes = yafgpu_image_bytes(desc->format, desc->image_width, desc->image_height);
	if(bytes == 0 || bytes > ((uint64_t)1 << 32)) return fail(-10, "film to image: image size or format out of range");
	HIP_OK(s->rt_image.reserve((size_t)bytes, nullptr));
	const int rc = yafgpu_film_to_image(s->rt_film, desc, s->rt_image, nullptr);
	if(rc) return rc;
	HIP_OK(hipMemcpy(h_image, s->rt_image, (size_t)bytes, hipMemcpyDeviceToHost));
	return 0;
}

int yafgpu_render_to_host(yafgpu_scene_t *s, const yafgpu_render_params *rp, float *h_film, yafgpu_counters *h_counters)
{
	if(!s || !rp || !h_film) return fail(-1, "null argument");
	if(rp->width <= 0 || rp->height <= 0) return fail(-10, "empty image");
	float *d_planes = nullptr, *d_film = nullptr; yafgpu_counters *d_cnt = nullptr;
	const size_t film_bytes = (size_t)rp->width * (size_t)rp->height * YAFGPU_FILM_CHANNELS * sizeof(float);
	s->rt_film_w = s->rt_film_h = 0;
	int rc = render_targets(s, rp->width, rp->height, &d_planes, &d_film, &d_cnt);
	if(rc) return rc;
	HIP_OK(hipMemset(d_cnt, 0, sizeof(yafgpu_counters)));
	rc = yafgpu_render_tiles(s, rp, d_planes, d_cnt, nullptr);
	if(!rc) rc = yafgpu_film_combine(d_planes, d_film, rp->width, rp->height, nullptr);
	if(!rc)
	{
		hipError_t e = hipDeviceSynchronize();
		if(e != hipSuccess) rc = fail(-100, std::string("render: ") + hipGetErrorString(e));
	}
	if(!rc)
	{
		if(hipMemcpy(h_film, d_film, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-100, "film download failed");
		if(h_counters && hipMemcpy(h_counters, d_cnt, sizeof(yafgpu_counters), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-100, "counter download failed");
	}
	if(!rc) { s->rt_film_w = rp->width; s->rt_film_h = rp->height; }
	return rc;
}

// ---- multi-pass anti-aliasing: TiledIntegrator::render (integrator_tiled.cc:116-258) -----------------------------
// The noise detection between passes (ImageFilm::nextPass, imagefilm.cc:270-480) is an image-space pass over the
// film so far: aa_detect_kernel below; next_pass_mask is the same on the host (YAFGPU_AA_DETECT=host), kept as its checker.
namespace {
__host__ __device__ float dark_threshold_curve(float b)   // ImageFilm::darkThresholdCurveInterpolate, imagefilm.cc:1312-1328
{
	if(b <= 0.10f) return 0.0001f;
	else if(b > 0.10f && b <= 0.20f) return (0.0001f + (b - 0.10f) * (0.0010f - 0.0001f) / 0.10f);
	else if(b > 0.20f && b <= 0.30f) return (0.0010f + (b - 0.20f) * (0.0020f - 0.0010f) / 0.10f);
	else if(b > 0.30f && b <= 0.40f) return (0.0020f + (b - 0.30f) * (0.0035f - 0.0020f) / 0.10f);
	else if(b > 0.40f && b <= 0.50f) return (0.0035f + (b - 0.40f) * (0.0055f - 0.0035f) / 0.10f);
	else if(b > 0.50f && b <= 0.60f) return (0.0055f + (b - 0.50f) * (0.0075f - 0.0055f) / 0.10f);
	else if(b > 0.60f && b <= 0.70f) return (0.0075f + (b - 0.60f) * (0.0100f - 0.0075f) / 0.10f);
	else if(b > 0.70f && b <= 0.80f) return (0.0100f + (b - 0.70f) * (0.0150f - 0.0100f) / 0.10f);
	else if(b > 0.80f && b <= 0.90f) return (0.0150f + (b - 0.80f) * (0.0250f - 0.0150f) / 0.10f);
	else if(b > 0.90f && b <= 1.00f) return (0.0250f + (b - 0.90f) * (0.0400f - 0.0250f) / 0.10f);
	else if(b > 1.00f && b <= 1.20f) return (0.0400f + (b - 1.00f) * (0.0800f - 0.0400f) / 0.20f);
	else if(b > 1.20f && b <= 1.40f) return (0.0800f + (b - 1.20f) * (0.0950f - 0.0800f) / 0.20f);
	else if(b > 1.40f && b <= 1.80f) return (0.0950f + (b - 1.40f) * (0.1000f - 0.0950f) / 0.40f);
	else return 0.1000f;
}
struct Px { float c[4]; };
__host__ __device__ Px px_normalized(const float *p)   // Pixel::normalized, util_image_buffers.h:39-43; Rgba / float, color.h:310-314
{
	Px o;
	if(p[4] != 0.f) { const float f = (float)(1.0 / (double)p[4]); for(int k = 0; k < 4; ++k) o.c[k] = p[k] * f; }
	else for(int k = 0; k < 4; ++k) o.c[k] = 0.f;
	return o;
}
__host__ __device__ float px_difference(const Px &a, const Px &b, bool use_rgb)   // Rgba::colorDifference, color.h:447-464
{
	const float bri_a = 0.2126f * a.c[0] + 0.7152f * a.c[1] + 0.0722f * a.c[2];
	const float bri_b = 0.2126f * b.c[0] + 0.7152f * b.c[1] + 0.0722f * b.c[2];
	float d = fabsf(bri_b - bri_a);
	if(use_rgb) for(int k = 0; k < 4; ++k) { const float dk = fabsf(b.c[k] - a.c[k]); if(d < dk) d = dk; }
	return d;
}
// which pixels get more samples; returns their number
int next_pass_mask(const float *film, int w, int h, const yafgpu_aa_schedule &aa, float aa_thesh, std::vector<uint8_t> &flags)
{
	flags.assign((size_t)w * (size_t)h, 0);
	if(!(aa_thesh > 0.f)) { std::fill(flags.begin(), flags.end(), (uint8_t)1); return w * h; }   // :319,460; doMoreSamples :919
	const int half = aa.variance_edge_size / 2;
	float scaled = aa_thesh;
	auto P = [&](int x, int y) { return film + 5 * ((size_t)y * (size_t)w + (size_t)x); };
	auto set = [&](int x, int y) { flags[(size_t)y * (size_t)w + (size_t)x] = 1; };
	const bool rgb = aa.detect_color_noise != 0;
	for(int y = 0; y < h - 1; ++y)
		for(int x = 0; x < w - 1; ++x)
		{
			if(P(x, y)[4] <= 0.f) set(x, y);
			const Px c = px_normalized(P(x, y));
			const float bri = 0.2126f * std::fabs(c.c[0]) + 0.7152f * std::fabs(c.c[1]) + 0.0722f * std::fabs(c.c[2]);
			if(aa.dark_detection_type == 1 && aa.dark_threshold_factor > 0.f) scaled = aa_thesh * ((1.f - aa.dark_threshold_factor) + (bri * aa.dark_threshold_factor));
			else if(aa.dark_detection_type == 2) scaled = dark_threshold_curve(bri);
			if(px_difference(c, px_normalized(P(x + 1, y)), rgb) >= scaled) { set(x, y); set(x + 1, y); }
			if(px_difference(c, px_normalized(P(x, y + 1)), rgb) >= scaled) { set(x, y); set(x, y + 1); }
			if(px_difference(c, px_normalized(P(x + 1, y + 1)), rgb) >= scaled) { set(x, y); set(x + 1, y + 1); }
			if(x > 0 && px_difference(c, px_normalized(P(x - 1, y + 1)), rgb) >= scaled) { set(x, y); set(x - 1, y + 1); }
			if(aa.variance_pixels > 0)
			{
				int vx = 0, vy = 0;
				for(int xd = -half; xd < half - 1; ++xd)
				{
					int xi = x + xd; if(xi < 0) xi = 0; else if(xi >= w - 1) xi = w - 2;
					if(px_difference(px_normalized(P(xi, y)), px_normalized(P(xi + 1, y)), rgb) >= scaled) ++vx;
				}
				for(int yd = -half; yd < half - 1; ++yd)
				{
					int yi = y + yd; if(yi < 0) yi = 0; else if(yi >= h - 1) yi = h - 2;
					if(px_difference(px_normalized(P(x, yi)), px_normalized(P(x, yi + 1)), rgb) >= scaled) ++vy;
				}
				if(vx + vy >= aa.variance_pixels)
					for(int xd = -half; xd < half; ++xd)
						for(int yd = -half; yd < half; ++yd)
						{
							int xi = x + xd; if(xi < 0) xi = 0; else if(xi >= w) xi = w - 1;
							int yi = y + yd; if(yi < 0) yi = 0; else if(yi >= h) yi = h - 1;
							set(xi, yi);
						}
			}
		}
	int n = 0;
	for(uint8_t f : flags) n += f;
	return n;
}
// The same on the device, one thread per pixel of the loop above (every store is the same 1: the order does not matter), on the
// combined film that is on the device anyway — the host version costs 10 ms per pass at 1024 x 1024 plus the film's way down.
__global__ __launch_bounds__(kBlock) void aa_detect_kernel(const float *film, int w, int h, yafgpu_aa_schedule aa, float aa_thesh, uint8_t *flags)
{
	const int n = (w - 1) * (h - 1);
	const int half = aa.variance_edge_size / 2;
	const bool rgb = aa.detect_color_noise != 0;
	for(int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
	{
		const int x = i % (w - 1), y = i / (w - 1);
		auto P = [&](int px, int py) { return film + 5 * ((size_t)py * (size_t)w + (size_t)px); };
		auto set = [&](int px, int py) { flags[(size_t)py * (size_t)w + (size_t)px] = 1; };
		float scaled = aa_thesh;
		if(P(x, y)[4] <= 0.f) set(x, y);
		const Px c = px_normalized(P(x, y));
		const float bri = 0.2126f * fabsf(c.c[0]) + 0.7152f * fabsf(c.c[1]) + 0.0722f * fabsf(c.c[2]);
		if(aa.dark_detection_type == 1 && aa.dark_threshold_factor > 0.f) scaled = aa_thesh * ((1.f - aa.dark_threshold_factor) + (bri * aa.dark_threshold_factor));
		else if(aa.dark_detection_type == 2) scaled = dark_threshold_curve(bri);
		if(px_difference(c, px_normalized(P(x + 1, y)), rgb) >= scaled) { set(x, y); set(x + 1, y); }
		if(px_difference(c, px_normalized(P(x, y + 1)), rgb) >= scaled) { set(x, y); set(x, y + 1); }
		if(px_difference(c, px_normalized(P(x + 1, y + 1)), rgb) >= scaled) { set(x, y); set(x + 1, y + 1); }
		if(x > 0 && px_difference(c, px_normalized(P(x - 1, y + 1)), rgb) >= scaled) { set(x, y); set(x - 1, y + 1); }
		if(aa.variance_pixels > 0)
		{
			int vx = 0, vy = 0;
			for(int xd = -half; xd < half - 1; ++xd)
			{
				int xi = x + xd; if(xi < 0) xi = 0; else if(xi >= w - 1) xi = w - 2;
				if(px_difference(px_normalized(P(xi, y)), px_normalized(P(xi + 1, y)), rgb) >= scaled) ++vx;
			}
			for(int yd = -half; yd < half - 1; ++yd)
			{
				int yi = y + yd; if(yi < 0) yi = 0; else if(yi >= h - 1) yi = h - 2;
				if(px_difference(px_normalized(P(x, yi)), px_normalized(P(x, yi + 1)), rgb) >= scaled) ++vy;
			}
			if(vx + vy >= aa.variance_pixels)
				for(int xd = -half; xd < half; ++xd)
					for(int yd = -half; yd < half; ++yd)
					{
						int xi = x + xd; if(xi < 0) xi = 0; else if(xi >= w) xi = w - 1;
						int yi = y + yd; if(yi < 0) yi = 0; else if(yi >= h) yi = h - 1;
						set(xi, yi);
					}
		}
	}
}
// A resumed render's start (yafgpu_aa_schedule::resume_film): the films summed in d_film in the order they are handed out, then the
// planes seeded from the sum.  One film goes in as it is.
int seed_resumed_planes(yafgpu_scene *s, const yafgpu_aa_schedule &aa, int w, int h, float *d_planes, float *d_film)
{
	const size_t n = (size_t)w * (size_t)h * YAFGPU_FILM_CHANNELS;
	const uint32_t grid = (uint32_t)std::min<size_t>((n + kBlock - 1) / kBlock, 2048);
	if(!aa.resume_next) HIP_OK(hipMemcpy(d_film, aa.resume_film, n * sizeof(float), hipMemcpyHostToDevice));
	else
	{
		DevMem<float> d_in;
		if(d_in.alloc(n) != hipSuccess) return fail(-3, "out of device memory (film merge)");
		std::vector<float> next;
		const float *src = aa.resume_film;
		for(int first = 1;; first = 0)
		{
			HIP_OK(hipMemcpy(d_in, src, n * sizeof(float), hipMemcpyHostToDevice));
			hipLaunchKernelGGL(film_add_kernel, dim3(grid), dim3(kBlock), 0, nullptr, d_film, (const float *)d_in.p, n, first);
			HIP_OK(hipGetLastError());
			if(next.empty())
			{
				try { next.resize(n); }
				catch(const std::bad_alloc &) { return fail(-3, "out of host memory (film merge)"); }
			}
			const int got = aa.resume_next(aa.resume_user, next.data(), (uint64_t)n);
			if(got < 0) return fail(-32, "the film source of a resumed render reported a failure");
			if(got == 0) break;
			src = next.data();
		}
	}
	hipLaunchKernelGGL(seed_planes_kernel, dim3(grid), dim3(kBlock), 0, nullptr, (const float *)d_film, d_planes, n);
	HIP_OK(hipGetLastError());
	// correlative_sample_number_ starts a render at zero (integrator_tiled.cc:192-194); the pass that would reset it does not run
	s->lc_host_counter = 0u;
	HIP_OK(s->rp_counter.reserve(1, nullptr));
	HIP_OK(hipMemsetAsync(s->rp_counter, 0, sizeof(uint32_t), nullptr));
	HIP_OK(hipDeviceSynchronize());
	return 0;
}
} // namespace

int yafgpu_render_passes_to_host(yafgpu_scene_t *s, const yafgpu_render_params *rp_in, const yafgpu_aa_schedule *aa_in,
                                 float *h_film, yafgpu_counters *h_counters, int32_t *resampled_out)
{
	if(!s || !rp_in || !h_film) return fail(-1, "null argument");
	yafgpu_aa_schedule aa{};
	if(aa_in) aa = *aa_in;
	if(aa.passes < 1) aa.passes = 1;
	const bool exchange = aa.passes > 1 && rp_in->shard_count > 1;
	if(exchange && !s->exchange) return fail(-16, "multi-pass anti-aliasing on a sharded frame needs an exchange function (yafgpu_scene_set_exchange): the noise detection between passes reads every pixel");
	const bool resumed = aa.resume_film != nullptr;
	if(resumed && rp_in->shard_count > 1) return fail(-17, "a resumed render of a sharded frame is not supported: a loaded film is a film of the whole frame");
	yafgpu_render_params rp = *rp_in;
	const int w = rp.width, h = rp.height;
	if(w <= 0 || h <= 0) return fail(-10, "empty image");
	float *d_planes = nullptr, *d_film = nullptr; yafgpu_counters *d_cnt = nullptr;
	const size_t film_bytes = (size_t)w * (size_t)h * YAFGPU_FILM_CHANNELS * sizeof(float);
	s->rt_film_w = s->rt_film_h = 0;
	{ const int rc_t = render_targets(s, w, h, &d_planes, &d_film, &d_cnt); if(rc_t) return rc_t; }
	HIP_OK(hipMemset(d_cnt, 0, sizeof(yafgpu_counters)));
	auto film_now = [&](bool download = true) -> int {
		int rc = yafgpu_film_combine(d_planes, d_film, w, h, nullptr);
		if(!rc && download && hipMemcpy(h_film, d_film, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-100, "film download failed");
		return rc;
	};
	// the whole frame's film for the detection step of a sharded render: all ranks' planes summed (exactly: one writer per
	// element), then combined in the single-GPU order
	DevMem<float> d_all;
	const size_t plane_floats = yafgpu_planes_bytes(w, h) / sizeof(float);
	auto film_of_all_ranks = [&](bool download = true) -> int {
		if(!d_all.p && d_all.alloc(plane_floats) != hipSuccess) return fail(-3, "out of device memory (plane exchange)");
		if(hipMemcpy(d_all, d_planes, plane_floats * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) return fail(-100, "plane copy failed");
		if(hipDeviceSynchronize() != hipSuccess) return fail(-100, "render failed before the plane exchange");
		if(s->exchange(s->exchange_user, d_all, (uint64_t)plane_floats)) return fail(-31, "the plane exchange function reported a failure");
		int rc = yafgpu_film_combine(d_all, d_film, w, h, nullptr);
		if(!rc && download && hipMemcpy(h_film, d_film, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-100, "film download failed");
		return rc;
	};
	// the detection step on the film that d_film holds: flags down (1 byte per pixel), counted here; < 0: error
	const bool detect_on_host = [] { const char *e = std::getenv("YAFGPU_AA_DETECT"); return e && std::strcmp(e, "host") == 0; }();
	auto detect = [&](float aa_thesh, std::vector<uint8_t> &flags) -> int {
		const size_t n_px = (size_t)w * (size_t)h;
		flags.assign(n_px, 0);
		if(!(aa_thesh > 0.f)) { std::fill(flags.begin(), flags.end(), (uint8_t)1); return w * h; }   // imagefilm.cc:319,460; doMoreSamples :919
		if(s->rt_flags.reserve(n_px, nullptr) != hipSuccess) return fail(-3, "out of device memory (resample flags)");
		if(hipMemsetAsync(s->rt_flags, 0, n_px, nullptr) != hipSuccess) return fail(-100, "flag reset failed");
		if(w > 1 && h > 1)
		{
			const uint32_t grid = (uint32_t)std::min<size_t>(((size_t)(w - 1) * (size_t)(h - 1) + kBlock - 1) / kBlock, 4096);
			hipLaunchKernelGGL(aa_detect_kernel, dim3(grid), dim3(kBlock), 0, nullptr, (const float *)d_film, w, h, aa, aa_thesh, s->rt_flags.p);
			if(hipGetLastError() != hipSuccess) return fail(-100, "detection kernel launch failed");
		}
		if(hipMemcpy(flags.data(), s->rt_flags, n_px, hipMemcpyDeviceToHost) != hipSuccess) return fail(-100, "flag download failed");
		int n = 0;
		for(uint8_t f : flags) n += f;
		return n;
	};
	// integrator_tiled.cc:136-258
	const int aa_samples = std::max(1, rp.aa_minsamples);
	const int aa_inc = aa.inc_samples > 0 ? aa.inc_samples : aa_samples;       // scene.cc:765
	float threshold = aa.threshold, sample_mult = 1.f, light_mult = 1.f;
	const int floor_pixels = (int)std::floor(aa.resampled_floor * (float)(w * h) / 100.f);
	rp.aa_minsamples = aa_samples; rp.multi_pass = aa.passes > 1 ? 1 : 0; rp.pass_offset = 0u; rp.accumulate = 0; rp.resample_mask = nullptr;
	if(aa.passes > 1) rp.aa_light_sample_multiplier = light_mult;
	// the libc rand() stream the tile seeds come from (integrator_tiled.cc:319): one value per tile per pass that runs, after
	// the values the last Material / ObjectGeometric constructor consumed (aa.rand_skip)
	std::vector<int32_t> rand_stream;
	const int n_tiles_frame = ((w + rp.tile_size - 1) / std::max(rp.tile_size, 1)) * ((h + rp.tile_size - 1) / std::max(rp.tile_size, 1));
	size_t rand_pos = (size_t)std::max(aa.rand_skip, 0);
	if(aa.rand_srand >= 0 && rp.tile_size > 0)
	{
		rand_stream.resize(rand_pos + (size_t)n_tiles_frame * (size_t)aa.passes);
		yafgpu_glibc_rand((uint32_t)aa.rand_srand, (int32_t)rand_stream.size(), rand_stream.data());
		rp.tile_rand = rand_stream.data() + rand_pos; rand_pos += (size_t)n_tiles_frame;
	}
	// A resumed render skips the first pass (integrator_tiled.cc:198-202: renderPass with 0 samples): no path work, no camera samples;
	// its tile seeds, taken above, are spent all the same (renderTile's first statement, :319)
	int rc = resumed ? seed_resumed_planes(s, aa, w, h, d_planes, d_film) : yafgpu_render_tiles(s, &rp, d_planes, d_cnt, nullptr);
	if(resampled_out) resampled_out[0] = resumed ? 0 : w * h;
	std::vector<uint8_t> mask;
	int acum = resumed ? (int)aa.resume_sampling_offset : aa_samples, resampled = 0; bool threshold_changed = true;
	for(int i = 1; i < aa.passes && !rc; ++i)
	{
		if(s->aborted()) { rc = fail(-30, "aborted"); break; }
		sample_mult *= aa.sample_multiplier_factor;
		light_mult *= aa.light_sample_multiplier_factor;
		if(!(resampled <= 0 && !threshold_changed))
		{
			if((rc = exchange ? film_of_all_ranks(detect_on_host) : film_now(detect_on_host))) break;
			if(detect_on_host) resampled = next_pass_mask(h_film, w, h, aa, threshold, mask);
			else if((resampled = detect(threshold, mask)) < 0) { rc = resampled; break; }
			threshold_changed = false;
		}
		const int n = (int)std::ceil((float)aa_inc * sample_mult);
		if(resampled_out) resampled_out[i] = resampled > 0 ? resampled : 0;
		if(resampled > 0)
		{
			rp.aa_minsamples = n; rp.pass_offset = (uint32_t)acum; rp.accumulate = 1;
			rp.aa_light_sample_multiplier = light_mult;
			rp.resample_mask = threshold > 0.f ? mask.data() : nullptr;
			if(!rand_stream.empty()) { rp.tile_rand = rand_stream.data() + rand_pos; rand_pos += (size_t)n_tiles_frame; }
			rc = yafgpu_render_tiles(s, &rp, d_planes, d_cnt, nullptr);
		}
		acum += n;
		if(resampled < floor_pixels)
		{
			const float ratio = std::min(8.f, ((float)floor_pixels / (float)resampled));
			threshold *= (1.f - 0.1f * ratio);
			if(threshold > 0.f) threshold_changed = true;
		}
	}
	if(!rc) rc = film_now();
	if(!rc)
	{
		hipError_t e = hipDeviceSynchronize();
		if(e != hipSuccess) rc = fail(-100, std::string("render: ") + hipGetErrorString(e));
	}
	if(!rc && h_counters && hipMemcpy(h_counters, d_cnt, sizeof(yafgpu_counters), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(-100, "counter download failed");
	if(!rc) { s->rt_film_w = w; s->rt_film_h = h; }
	return rc;
}

// Ray batches (tests and kernel-level measurements): Scene::intersect / Scene::isShadowed on arrays, answered by the traversal
// kernel of the wavefront pass.  Ray i is path slot i of a pass without queues (the identity): record 0 holds (from, tmin),
// record 1 (dir, tmax); a closest hit is answered in record 2, an occluded ray sets verdict bit 4 i.  wf_trace reads the top two
// bits of a queue entry as tags, so the rays go in chunks of kWfMaxPaths at most.  No counters and no transparent shadows
// (rp.transp_shad = 0): the any-hit ray is intersectS from 0.
static int trace_batch(yafgpu_scene_t *s, int32_t n, const float *rays, int32_t *tri, float *t, float *bary, int32_t *shadowed, bool any)
{
	if(!s || !rays || n < 0) return fail(-1, "bad argument");
	if(n == 0) return 0;
	int rc = device_cus(s);
	if(rc) return rc;
	const uint32_t cap = std::min((uint32_t)n, kWfMaxPaths);
	DevMem<float4> d_state; DevMem<uint32_t> d_cnt, d_verdict;
	HIP_OK(d_state.alloc((size_t)3 * cap));
	HIP_OK(d_cnt.alloc(5));
	HIP_OK(d_verdict.alloc(((size_t)4 * cap + 31) / 32));
	std::vector<float4> h((size_t)2 * cap);
	std::vector<uint32_t> h_verdict;
	WfArgs a{};
	a.ra.sc = s->dev;
	a.state = d_state; a.cap = cap;
	a.cnt_in = d_cnt; a.verdict = d_verdict;
	const void *kernel = any ? (const void *)wf_trace<true, false> : (const void *)wf_trace<false, false>;
	const int grid = wf_grid(kernel, s->n_cus, read_switches(), true);
	g_trace_grid[any ? 1 : 0] = grid;
	for(uint32_t o = 0; o < (uint32_t)n; o += cap)
	{
		const uint32_t m = std::min(cap, (uint32_t)n - o);
		for(uint32_t i = 0; i < m; ++i)
		{
			const float *r = rays + 8 * (size_t)(o + i);
			h[i] = make_float4(r[0], r[1], r[2], r[6]);
			h[cap + i] = make_float4(r[3], r[4], r[5], r[7]);
		}
		HIP_OK(hipMemcpy(d_state, h.data(), h.size() * sizeof(float4), hipMemcpyHostToDevice));
		const uint32_t cnt[5] = {m, m, 0u, 0u, 0u};
		HIP_OK(hipMemcpy(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
		const size_t words = ((size_t)4 * m + 31) / 32;
		if(any) HIP_OK(hipMemset(d_verdict, 0, words * sizeof(uint32_t)));
		if(any) hipLaunchKernelGGL((wf_trace<true, false>), dim3(grid), dim3(kBlock), 0, nullptr, a);
		else hipLaunchKernelGGL((wf_trace<false, false>), dim3(grid), dim3(kBlock), 0, nullptr, a);
		HIP_OK(hipGetLastError());
		HIP_OK(hipDeviceSynchronize());
		if(any)
		{
			h_verdict.resize(words);
			HIP_OK(hipMemcpy(h_verdict.data(), d_verdict, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
			for(uint32_t i = 0; i < m; ++i) shadowed[o + i] = (int32_t)((h_verdict[i >> 3] >> (4u * (i & 7u))) & 1u);
			continue;
		}
		HIP_OK(hipMemcpy(h.data(), d_state + (size_t)2 * cap, m * sizeof(float4), hipMemcpyDeviceToHost));
		for(uint32_t i = 0; i < m; ++i)
		{	// (tri, t, u, v); tri -1: a miss
			const float4 ans = h[i];
			int32_t ti; std::memcpy(&ti, &ans.x, sizeof ti);
			const bool hit = ti >= 0;
			const size_t k = o + i;
			tri[k] = hit ? ti : -1; t[k] = hit ? ans.y : 0.f;
			bary[3 * k] = hit ? 1.f - ans.z - ans.w : 0.f; bary[3 * k + 1] = hit ? ans.z : 0.f; bary[3 * k + 2] = hit ? ans.w : 0.f;
		}
	}
	return 0;
}

int yafgpu_trace_closest(yafgpu_scene_t *s, int32_t n, const float *rays, int32_t *tri, float *t, float *bary)
{
	if(!tri || !t || !bary) return fail(-1, "null output");
	return trace_batch(s, n, rays, tri, t, bary, nullptr, false);
}
int yafgpu_trace_shadow(yafgpu_scene_t *s, int32_t n, const float *rays, int32_t *shadowed)
{
	if(!shadowed) return fail(-1, "null output");
	return trace_batch(s, n, rays, nullptr, nullptr, nullptr, shadowed, true);
}

uint32_t yafgpu_trace_reservation(uint32_t n, uint32_t seen, uint32_t waves) { return waves ? trace_reservation(n, seen, waves) : 0u; }
void yafgpu_trace_schedule(uint32_t info[8])
{
	info[0] = (uint32_t)YAFGPU_TRACE_BATCH_MIN; info[1] = (uint32_t)YAFGPU_TRACE_BATCH; info[2] = (uint32_t)YAFGPU_TRACE_BATCH_DIV;
	info[3] = (uint32_t)YAFGPU_TRACE_BATCH_SHRINK; info[4] = (uint32_t)YAFGPU_TRACE_STATIC_FIRST; info[5] = (uint32_t)kWavesPerBlock;
	info[6] = (uint32_t)g_trace_grid[0].load(); info[7] = (uint32_t)g_trace_grid[1].load();
}

#if YAFGPU_TRACE_EXIT_LOG
// (measurement build) the traversal waves' exit records so far: copies up to `cap` of them (8 words each) to `out`, empties the log
// if `reset`, and returns how many there were
int yafgpu_exit_log_read(uint32_t *out, uint32_t cap, int reset)
{
	uint32_t n = 0u;
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_exit_log_n), sizeof n));
	n = std::min(n, kExitLogCap);
	if(out && std::min(n, cap)) HIP_OK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_exit_log), (size_t)std::min(n, cap) * 2u * sizeof(uint4)));
	const uint32_t zero = 0u;
	if(reset) HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(g_exit_log_n), &zero, sizeof zero));
	return (int)n;
}
#endif

void yafgpu_glibc_rand(uint32_t seed, int32_t count, int32_t *out)
{	// glibc stdlib/random_r.c, TYPE_3: 31 words seeded by the Lehmer generator 16807 x mod 2^31 - 1 (Schrage's method), then
	// r[i] = r[i-3] + r[i-31]; the first 310 values are discarded; rand() returns r >> 1
	if(count <= 0 || !out) return;
	std::vector<uint32_t> r((size_t)count + 344);
	if(seed == 0u) seed = 1u;
	r[0] = seed;
	for(int i = 1; i < 31; ++i)
	{
		int32_t word = (int32_t)r[(size_t)i - 1];
		const long hi = word / 127773, lo = word % 127773;
		word = (int32_t)(16807 * lo - 2836 * hi);
		if(word < 0) word += 2147483647;
		r[(size_t)i] = (uint32_t)word;
	}
	for(size_t i = 31; i < 34; ++i) r[i] = r[i - 31];
	for(size_t i = 34; i < r.size(); ++i) r[i] = r[i - 31] + r[i - 3];
	for(int32_t k = 0; k < count; ++k) out[k] = (int32_t)(r[(size_t)k + 344] >> 1);
}

int yafgpu_scene_set_exchange(yafgpu_scene_t *s, yafgpu_exchange_fn fn, void *user)
{
	if(!s) return fail(-1, "null argument");
	s->exchange = fn; s->exchange_user = user;
	return 0;
}

int yafgpu_scene_set_abort_flag(yafgpu_scene_t *s, const volatile int32_t *flag)
{
	if(!s) return fail(-1, "null argument");
	s->abort_flag = flag;
	return 0;
}

int yafgpu_scene_set_pass_pipelining(yafgpu_scene_t *s, int32_t mode)
{
	if(!s) return fail(-1, "null scene");
	s->pass_pipelining = mode < 0 ? -1 : (mode != 0 ? 1 : 0);
	return 0;
}
int yafgpu_set_profiling(yafgpu_scene_t *s, int32_t enable)
{
	if(!s) return fail(-1, "null argument");
	s->profiling = enable != 0;
	return 0;
}
int yafgpu_get_profile(const yafgpu_scene_t *s, double ms[4], uint64_t launches[4])
{
	if(!s) return fail(-1, "null argument");
	for(int k = 0; k < 4; ++k) { ms[k] = s->prof_ms[k]; launches[k] = s->prof_launches[k]; }
	return 0;
}

int yafgpu_probe(yafgpu_scene_t *s, int32_t op, int32_t n, const float *in, int32_t n_in, float *out, int32_t n_out)
{
	if(!s || !in || !out || n < 0 || n_in <= 0 || n_out <= 0) return fail(-1, "bad argument");
	if(n == 0) return 0;
	DevMem<float> d_in, d_out;
	HIP_OK(d_in.alloc((size_t)n * (size_t)n_in));
	HIP_OK(d_out.alloc((size_t)n * (size_t)n_out));
	HIP_OK(hipMemcpy(d_in, in, (size_t)n * (size_t)n_in * sizeof(float), hipMemcpyHostToDevice));
	HIP_OK(hipMemset(d_out, 0, (size_t)n * (size_t)n_out * sizeof(float)));
	hipLaunchKernelGGL(probe_kernel, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, s->dev, op, n, d_in.p, n_in, d_out.p, n_out);
	HIP_OK(hipGetLastError());
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipMemcpy(out, d_out, (size_t)n * (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost));
	return 0;
}

} // extern "C"
#endif // YAFGPU_VARIANT_TU
