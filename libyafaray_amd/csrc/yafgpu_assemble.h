// Scene rows of instanced geometry and of curve meshes, made on the device (yafgpu_assemble.hip): what yafgpu_scene_create launches when
// its descriptor has segments (include/yafgpu.h, yafgpu_instancing).  Every pointer is a device pointer; an optional array is nullptr.
#ifndef YAFGPU_ASSEMBLE_H
#define YAFGPU_ASSEMBLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/yafgpu.h"

namespace yafgpu {

struct AssembleArgs
{
	const yafgpu_segment *segs;      // n_segs segments, ranges checked by the caller
	const uint32_t *seg_first;       // n_segs + 1: exclusive prefix of the segments' triangle counts, seg_first[n_segs] = n_out
	int n_segs;
	uint32_t n_out;
	// the descriptor's own arrays (plain segments)
	const float *p_verts; const int32_t *p_mat; const float *p_vn, *p_uv, *p_orco;
	// the base pools (instance segments)
	const float *b_verts; const int32_t *b_mat; const float *b_vn; const uint8_t *b_vn0; const float *b_uv, *b_orco;
	// the curve point pool (curve segments): x y z h s per point
	const float *c_points;
	const yafgpu_material *mats;     // the scene's material table: a record's visibility rides in its triangles' records
	// outputs, n_out rows each
	float4 *rec;                     // 3 per row: (a, eps) (e1, mat | vis << 30) (e2, 0)
	float4 *ng;                      // (geometric normal, smooth flag)
	float4 *vn;                      // 3 per row, or nullptr
	float *uv, *orco;                // 6 / 9 per row, or nullptr
	float *e3;                       // 3 per row (c - b, bump mapping), or nullptr
	float *verts;                    // 9 per row: what the tree builders take
};

// one launch on the null stream; the caller synchronises.  hipSuccess or the launch error.
hipError_t assemble_rows(const AssembleArgs &a);

} // namespace yafgpu
#endif
