// Scene set-up for instanced geometry on the MI355X (gfx950): every row of the triangle, shading and texture-coordinate arrays, made on
// the device from the plain meshes, the base meshes and the instances' matrices.
//
// The reference does not trace instances through a second level.  Scene::addInstance (scene.cc:1105-1130) makes a
// TriangleObjectInstance whose TriangleInstance triangles enter the same kd-tree as every other triangle (scene.cc:797-817); their
// vertices are obj_to_world * base vertex, and their edges and epsilon are cached from those vertices (triangle.h:210-220, :306-356).
// So an instance is more rows, and making them is the hot part of a scene with a thousand instances: one thread per output triangle
// here, instead of a serial host loop and an upload of the flattened arrays.
//
// A streaming kernel: no atomics, no LDS.  The arithmetic is the host loop's of yafgpu_scene_create, operation for operation: the unit
// is built with -ffp-contract=off and IEEE square root and division (csrc/build.sh; DESIGN §4 on __fsqrt_rn), the epsilon's product is
// taken in double, and the normalisations are Vec3::normalize (vector.h:227-238).
//
// A curve (Scene::endCurveMesh, scene.cc:154-281) is more rows too: the reference extrudes every point of a strand's poly-line into a
// triangular cross-section and fills a prism per segment, all of it an ordinary TriangleObject.  The host hands over the points with
// their two extrusion scales (its libm's pow is the reference's); a thread here makes one triangle of the prism from the up to six
// extruded points it touches.
#include "yafgpu_assemble.h"
#include "yafgpu_math.h"

namespace yafgpu {

namespace {

constexpr int kAssembleBlock = 256;      // like the device unit's other set-up kernels

struct A3 { float x, y, z; };
__device__ inline A3 sub3(const A3 &a, const A3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline A3 cross3(const A3 &a, const A3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// Vec3::normalize, vector.h:227-238
__device__ inline A3 normalize3(A3 v)
{
	float len = v.x * v.x + v.y * v.y + v.z * v.z;
	if(len != 0.f) { len = 1.0f / sqrtf(len); v.x *= len; v.y *= len; v.z *= len; }
	return v;
}
__device__ inline float length3(const A3 &v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }
// Matrix4 * Point3, matrix4.h:89-94: per row ((m0 * x + m1 * y) + m2 * z) + m3
__device__ inline A3 mul_point(const float *m, const A3 &p)
{
	return {m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7], m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]};
}
// Matrix4 * Vec3, matrix4.h:82-87: no translation
__device__ inline A3 mul_vec(const float *m, const A3 &v)
{
	return {m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z, m[8] * v.x + m[9] * v.y + m[10] * v.z};
}
__device__ inline A3 load3(const float *p) { return {p[0], p[1], p[2]}; }

// Scene::endCurveMesh's vertex extrusion, scene.cc:169-193: point i of a strand of n points at pool (5 floats per point: x y z h s) and its
// extruded points a = o - h * v - s * u, b = o - h * v + s * u.  (u, v) is createCs__ of the normalised tangent p[i + 1] - p[i]; the last
// point keeps the frame of the one before it (:181-186).  Coincident points leave the tangent zero, which takes createCs__'s z branch.
__device__ inline void curve_point(const float *pool, int i, int n, A3 &o, A3 &pa, A3 &pb)
{
	const int t = i < n - 1 ? i : n - 2;
	const A3 nn = normalize3(sub3(load3(pool + 5 * (size_t)(t + 1)), load3(pool + 5 * (size_t)t)));
	V3 u, v;
	create_cs(mk(nn.x, nn.y, nn.z), u, v);
	const float *q = pool + 5 * (size_t)i;
	o = load3(q);
	const float h = q[3], s = q[4];
	const A3 hv = {h * v.x, h * v.y, h * v.z}, su = {s * u.x, s * u.y, s * u.z};      // operator*(float, Vec3), vector.h:150-153
	const A3 m = sub3(o, hv);                                                         // Point3 - Vec3, :200-203
	pa = sub3(m, su);
	pb = {m.x + su.x, m.y + su.y, m.z + su.z};
}
// Row k of a strand of n points, in the order of the face fill (scene.cc:196-275): the bottom cap, six triangles per segment, the top cap.
// Corners and one texture coordinate per corner, (t, t): su = (float)j / (n - 1) at the segment's first point, sv = su + 1. / (n - 1), the
// sum in double, at its second.
__device__ inline void curve_row(const float *pool, int n, uint32_t k, A3 &va, A3 &vb, A3 &vc, float t[3])
{
	const uint32_t last = 6u * (uint32_t)(n - 1) + 1u;
	A3 o, pa, pb;
	if(k == 0u)
	{	// close bottom: Triangle(a_1, a_3, a_2), all three corners at UV 0
		curve_point(pool, 0, n, o, pa, pb);
		va = o; vb = pb; vc = pa;
		t[0] = t[1] = t[2] = (float)0 / (float)(n - 1);
		return;
	}
	const int j = k == last ? n - 2 : (int)((k - 1u) / 6u);
	const float su = (float)j / (float)(n - 1);
	const float sv = (float)((double)su + 1. / (double)(n - 1));
	if(k == last)
	{	// close top: Triangle(i, 2 * i + n, 2 * i + n + 1) at the last point, with the last segment's iv
		curve_point(pool, n - 1, n, o, pa, pb);
		va = o; vb = pa; vc = pb;
		t[0] = t[1] = t[2] = sv;
		return;
	}
	A3 o2, pa2, pb2;
	curve_point(pool, j, n, o, pa, pb);
	curve_point(pool, j + 1, n, o2, pa2, pb2);
	switch((k - 1u) % 6u)
	{
		case 0u: va = o; vb = pa2; vc = o2; t[0] = su; t[1] = sv; t[2] = sv; break;      // (a_1, b_2, b_1)
		case 1u: va = o; vb = pa; vc = pa2; t[0] = su; t[1] = su; t[2] = sv; break;      // (a_1, a_2, b_2)
		case 2u: va = pa; vb = pb2; vc = pa2; t[0] = su; t[1] = sv; t[2] = sv; break;    // (a_2, b_3, b_2)
		case 3u: va = pa; vb = pb; vc = pb2; t[0] = su; t[1] = su; t[2] = sv; break;     // (a_2, a_3, b_3)
		case 4u: va = pb2; vb = pb; vc = o; t[0] = sv; t[1] = su; t[2] = su; break;      // (b_3, a_3, a_1)
		default: va = pb2; vb = o; vc = o2; t[0] = sv; t[1] = su; t[2] = sv; break;      // (b_3, a_1, b_1)
	}
}

__global__ __launch_bounds__(kAssembleBlock) void assemble_kernel(const AssembleArgs a)
{
	const uint32_t i = blockIdx.x * (uint32_t)kAssembleBlock + threadIdx.x;
	if(i >= a.n_out) return;
	// the thread's segment: the last one whose first row is <= i (empty segments share their successor's first row and are passed over).
	// Wave-uniform except where a wave straddles a segment boundary.
	int lo = 0, hi = a.n_segs - 1;
	while(lo < hi)
	{
		const int mid = (lo + hi + 1) >> 1;
		if(a.seg_first[mid] <= i) lo = mid; else hi = mid - 1;
	}
	const yafgpu_segment &sg = a.segs[lo];
	const bool inst = sg.kind == YAFGPU_SEGMENT_INSTANCE, curve = sg.kind == YAFGPU_SEGMENT_CURVE;
	const size_t src = curve ? 0 : (size_t)sg.first + (size_t)(i - a.seg_first[lo]);      // a curve's rows have no source row
	const float *m = sg.m;

	A3 va, vb, vc;
	float ct[3] = {0.f, 0.f, 0.f};      // a curve row's texture coordinate per corner
	if(curve) curve_row(a.c_points + 5 * (size_t)sg.first, sg.count, i - a.seg_first[lo], va, vb, vc, ct);
	else
	{
		const float *pv = (inst ? a.b_verts : a.p_verts) + 9 * src;
		va = load3(pv); vb = load3(pv + 3); vc = load3(pv + 6);
	}
	A3 n;      // the geometric normal
	if(inst)
	{	// TriangleInstance::getNormal, triangle.h:376-379: Vec3(M * base normal).normalize(), the base normal being recNormal (:295-302) of the
		// base's own vertices.  Not recomputed from the transformed edges: under a mirroring matrix it points the other way, under
		// non-uniform scale it is not perpendicular to the triangle.
		const A3 nb = normalize3(cross3(sub3(vb, va), sub3(vc, va)));
		n = normalize3(mul_vec(m, nb));
		va = mul_point(m, va); vb = mul_point(m, vb); vc = mul_point(m, vc);
	}
	// Triangle / TriangleInstance::updateIntersectionCachedValues, triangle.h:197-220
	const A3 e1 = sub3(vb, va), e2 = sub3(vc, va);
	const float eps = (float)((double)0.1f * 0.00005 * (double)fmaxf(length3(e1), length3(e2)));
	if(!inst) n = normalize3(cross3(e1, e2));      // recNormal
	const uint32_t mat = curve ? sg.flags : (uint32_t)(inst ? a.b_mat : a.p_mat)[src];
	const uint32_t vis = (uint32_t)a.mats[mat].visibility & 3u;
	a.rec[3 * (size_t)i] = make_float4(va.x, va.y, va.z, eps);
	a.rec[3 * (size_t)i + 1] = make_float4(e1.x, e1.y, e1.z, __uint_as_float(mat | (vis << 30)));
	a.rec[3 * (size_t)i + 2] = make_float4(e2.x, e2.y, e2.z, 0.f);
	{
		float *ov = a.verts + 9 * (size_t)i;
		ov[0] = va.x; ov[1] = va.y; ov[2] = va.z; ov[3] = vb.x; ov[4] = vb.y; ov[5] = vb.z; ov[6] = vc.x; ov[7] = vc.y; ov[8] = vc.z;
	}
	if(a.e3 != nullptr) { float *o = a.e3 + 3 * (size_t)i; o[0] = vc.x - vb.x; o[1] = vc.y - vb.y; o[2] = vc.z - vb.z; }

	// vertex normals: a corner without one takes the geometric normal (Triangle::getSurface, triangle.cc:38-40).  An instance reads
	// them when the flags it copied say so, each as Vec3(M * normals_[index]) (object_geom_mesh.h:130), not normalised before the
	// barycentric sum, and its test is `index > 0` (triangle.cc:215-217): the corner whose normal has index 0 takes the geometric normal too.
	// A curve's object has none.
	const float *qn = curve ? nullptr : inst ? ((sg.flags & YAFGPU_INSTANCE_SMOOTH) != 0u ? a.b_vn : nullptr) : a.p_vn;
	A3 cn[3] = {n, n, n};
	bool smooth = false;
	if(qn != nullptr)
	{
		qn += 9 * src;
		const uint32_t index0 = inst ? (uint32_t)a.b_vn0[src] : 0u;
		for(int c = 0; c < 3; ++c)
		{
			const A3 q = load3(qn + 3 * c);
			if((q.x == 0.f && q.y == 0.f && q.z == 0.f) || ((index0 >> c) & 1u) != 0u) continue;
			cn[c] = inst ? mul_vec(m, q) : q;
			smooth = true;
		}
	}
	a.ng[i] = make_float4(n.x, n.y, n.z, __uint_as_float(smooth ? 1u : 0u));
	if(a.vn != nullptr)
		for(int c = 0; c < 3; ++c) a.vn[3 * (size_t)i + (size_t)c] = make_float4(cn[c].x, cn[c].y, cn[c].z, 0.f);

	// texture coordinates: the base's own values under the flags the instance copied (TriangleInstance::getSurface, triangle.cc:224-256);
	// a first word of NaN says "none" (orco = the hit point; no UVs)
	const float none = __uint_as_float(0x7fc00000u);
	if(a.uv != nullptr)
	{
		const float *q = inst ? ((sg.flags & YAFGPU_INSTANCE_UV) != 0u ? a.b_uv : nullptr) : a.p_uv;
		float *o = a.uv + 6 * (size_t)i;
		if(curve) for(int c = 0; c < 3; ++c) o[2 * c] = o[2 * c + 1] = ct[c];      // addUv(su, su) / addUv(sv, sv), scene.cc:205-206
		else if(q != nullptr) for(int k = 0; k < 6; ++k) o[k] = q[6 * src + (size_t)k];
		else { o[0] = none; for(int k = 1; k < 6; ++k) o[k] = 0.f; }
	}
	if(a.orco != nullptr)
	{
		const float *q = curve ? nullptr : inst ? ((sg.flags & YAFGPU_INSTANCE_ORCO) != 0u ? a.b_orco : nullptr) : a.p_orco;      // TriangleObject(.., has_uv = true, has_orco = false), scene.cc:142
		float *o = a.orco + 9 * (size_t)i;
		if(q != nullptr) for(int k = 0; k < 9; ++k) o[k] = q[9 * src + (size_t)k];
		else { o[0] = none; for(int k = 1; k < 9; ++k) o[k] = 0.f; }
	}
}

} // namespace

hipError_t assemble_rows(const AssembleArgs &a)
{
	if(a.n_out == 0u || a.n_segs <= 0) return hipSuccess;
	hipLaunchKernelGGL(assemble_kernel, dim3((a.n_out + (uint32_t)kAssembleBlock - 1u) / (uint32_t)kAssembleBlock), dim3(kAssembleBlock), 0, nullptr, a);
	return hipGetLastError();
}

} // namespace yafgpu
