// A scene-specialised build of the shading kernel (wf_shade).
//
// The shading kernel is one straight-line program over every material type and feature of the path; its register
// and scratch budget is set by the union of them all (168 VGPRs + 116 B of scratch at 3 waves per SIMD).  Scenes
// that use a subset run a kernel compiled for that subset: this file is compiled once per variant with
//
//   -DYAFGPU_VARIANT_NAME=<name>  -DYAFGPU_MAT_MASK=<bit per YAFGPU_MAT_* handled>  -DYAFGPU_LIGHT_MASK=<bit per YAFGPU_LIGHT_* handled>
//   -DYAFGPU_FEAT_RECURSE=<0|1>  [-DYAFGPU_FEAT_LIGHTS=0]  [-DYAFGPU_FEAT_MULTI=0]  [-DYAFGPU_FEAT_AO=0]
//
// (FEAT_LIGHTS=0: the program of a serial-state replay's RECORD pass — no light estimate, the vertex of a resume in registers)
// (FEAT_AO: ambient occlusion.  No variant has it — pick_shade_variant sends a render with do_AO to the main unit's general kernel — so
// the flag is 0 here whether or not the command line says so; asking for 1 is an error)
// (the exception is the unit built with the blend material's bit, YAFGPU_MAT_MASK & 0x100: the general kernel with BlendMaterial's code, which
// keeps every feature of the main unit's wf_shade — shader nodes, the anisotropic lobe, every light type, ambient occlusion — and is picked by
// a blend in use and nothing else, pick_shade_variant; and the two units built with the mesh light's bit, YAFGPU_LIGHT_MASK & 0x80, which are
// the general kernel and the blend's with that light's code, picked by a mesh light in the scene, and the two built with the portal light's
// bit as well, YAFGPU_LIGHT_MASK & 0x100, picked by a portal light, and the two built with the IES light's bits on top of those,
// YAFGPU_LIGHT_MASK & 0x600, picked by an IES light of either kind, and the two built with the spot light's bits on top of all of them,
// YAFGPU_LIGHT_MASK & 0x1800, picked by a spot light of either kind, and the two built with -DYAFGPU_FEAT_SKY=1 on top of those, which
// evaluate the gradient and sunsky backgrounds and are picked by such a background before anything else)
//
// and includes the main unit with everything but wf_shade and what it calls compiled out.  All of its symbols live in
// their own namespace (the macro below renames `yafgpu`), so the variants and the main unit link into one library; the
// main unit reaches a variant through the three C functions at the bottom (yafgpu_device.hip: shade_variants).
#ifndef YAFGPU_VARIANT_NAME
#error "compile with -DYAFGPU_VARIANT_NAME=..., -DYAFGPU_MAT_MASK=..., -DYAFGPU_LIGHT_MASK=..., -DYAFGPU_FEAT_RECURSE=..."
#endif
#ifndef YAFGPU_LIGHT_MASK
#error "compile with -DYAFGPU_LIGHT_MASK=... (the light types the variant handles)"
#endif
#ifndef YAFGPU_FEAT_AO
#define YAFGPU_FEAT_AO 0
#elif YAFGPU_FEAT_AO && !((YAFGPU_MAT_MASK) & 0x100u) && !((YAFGPU_LIGHT_MASK) & 0x80u)
#error "a shade variant with ambient occlusion: pick_shade_variant (yafgpu_device.hip) assumes that none has it"
#endif
#define YAFGPU_VARIANT_TU 1
#define YG_CAT2(a, b) a##b
#define YG_CAT(a, b) YG_CAT2(a, b)
#define yafgpu YG_CAT(yafgpu_shade_, YAFGPU_VARIANT_NAME)
#include "yafgpu_device.hip"

namespace vns = yafgpu;
#undef yafgpu

extern "C" {

// material types / light types / features this variant was compiled for
void YG_CAT(YG_CAT(yafgpu_shade_, YAFGPU_VARIANT_NAME), _describe)(uint32_t *mat_mask, int *recurse, int *lights, int *multi, uint32_t *light_mask)
{
	*mat_mask = (uint32_t)(YAFGPU_MAT_MASK); *recurse = YAFGPU_FEAT_RECURSE; *lights = YAFGPU_FEAT_LIGHTS; *multi = YAFGPU_FEAT_LIGHTS && YAFGPU_FEAT_MULTI;
	*light_mask = (uint32_t)(YAFGPU_LIGHT_MASK);
}
const void *YG_CAT(YG_CAT(yafgpu_shade_, YAFGPU_VARIANT_NAME), _kernel)() { return (const void *)vns::wf_shade; }
// args: the main unit's WfArgs (same definition, so the same layout)
int YG_CAT(YG_CAT(yafgpu_shade_, YAFGPU_VARIANT_NAME), _launch)(const void *args, size_t bytes, int grid, hipStream_t stream)
{
	vns::WfArgs a;
	if(bytes != sizeof a) return -1;
	std::memcpy(&a, args, sizeof a);
	hipLaunchKernelGGL(vns::wf_shade, dim3((unsigned)grid), dim3(vns::kBlock), 0, stream, a);
	return 0;       // the caller checks hipGetLastError like after its own launches
}

} // extern "C"
