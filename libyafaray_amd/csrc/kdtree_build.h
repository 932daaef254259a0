// Host-side SAH kd-tree builder producing the flattened, index-based tree the HIP traversal
// kernels walk.  This is NOT a mirror of the reference's builder (TriKdTree::buildTree,
// src/common/kdtree_triangle.cc:468-675, which depends on double-precision triangle clipping);
// only the results of closest-hit / any-hit queries are contractual.  It keeps
// the reference's build *parameters* (scene.cc:818, kdtree_triangle.cc:89-100).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace yafgpu {

// 8-byte node, interior and leaf alike.
//   interior: a = float bits of the split position, b = axis | (right_child_index << 2); the near
//             (left/below) child is always the next node in memory (depth-first layout)
//   leaf    : a = index of the first entry in the leaf-reference array, b = 3 | (prim_count << 2)
struct KdNode { uint32_t a, b; };

struct KdTree
{
	std::vector<KdNode> nodes;
	std::vector<uint32_t> refs;
	float bound_lo[3], bound_hi[3];
	int max_depth = 0;      // deepest leaf actually produced
	double build_seconds = 0;
};

// verts: n_tris*9 floats (a,b,c).  depth_cap bounds the tree depth (the traversal stack never
// needs more entries than the depth).  threads<=0: hardware concurrency.
void build_kdtree(const float *verts, int n_tris, int depth_cap, int threads, KdTree &out);

// The same tree built on the GPU (kdtree_build_device.hip): breadth-first binned / exact-candidate SAH with the same
// parameters and cost model.  Returns 0, or a negative code with *err set (never falls back to the host builder).
// returns 0, -1 (device error) or -2 (the arrays sized for `room` x 8 references per triangle overflowed)
int build_kdtree_device(const float *verts, int n_tris, int depth_cap, KdTree &out, std::string *err, int room = 1);
// the same with more room on -2 (1, 4, 16), for callers that want a device-built tree or an error
int build_kdtree_device_retry(const float *verts, int n_tris, int depth_cap, KdTree &out, std::string *err);

// The treelet layout of the same tree, the one the traversal kernels (wf_trace) walk: an interior node and its two children in
// one 32-byte record, read as two uint4, so that one fetch brings two levels of the walk.
//   words 0-3: split of the root, split of the left child, split of the right child (float bits, as in KdNode), header =
//              axis of the root | axis of the left child << 2 | axis of the right child << 4, where axis 3 marks a leaf child
//   words 4-7: links — [4], [5] the left child's two children, or [4] the left child itself when it is a leaf (then [5] is 0);
//              [6], [7] the same for the right child
// A link names the place of a walk:
//   bit 31 clear      a node of a treelet: treelet << 2 | slot (0 root, 1 left child, 2 right child)
//   bits 31:30 = 10   a leaf inline: first reference in bits 23:0, reference count in bits 29:24 (kLinkEmpty: an empty leaf)
//   bits 31:30 = 11   a leaf whose numbers do not fit inline: (first reference, count) at leaves[2 * (link & kLinkIndex)]
// The (up to four) treelets below a treelet take consecutive numbers, and subtrees are numbered left first.
constexpr uint32_t kLinkLeaf = 0x80000000u, kLinkEscape = 0x40000000u, kLinkIndex = 0x3fffffffu, kLinkEmpty = kLinkLeaf;
constexpr uint32_t kLinkFirstBits = 24u, kLinkCountMax = 63u;
struct TreeletLayout
{
	std::vector<uint32_t> words;      // 8 per treelet
	std::vector<uint32_t> leaves;     // 2 per escaped leaf
	uint32_t root = kLinkEmpty;       // where every walk starts: treelet 0, or the root leaf of a tree without interior nodes
};
// inline_leaves false sends every non-empty leaf to the escape array (a test aid).  Returns 0, or -2 when the tree has too many
// treelets or escaped leaves for the link's index bits.
int build_treelets(const std::vector<KdNode> &nodes, bool inline_leaves, TreeletLayout &out);

// The order of wf_trace's own copy of the triangle records: pos[t] is the rank of triangle t's first occurrence in the leaf
// references, which are in depth-first leaf order, so that leaves next to each other in space find their records next to each other
// in memory; triangles that no leaf references follow, in id order.  A permutation of [0, n_tris); O(refs).
//   refs 3 1 3 0 1 6 6 3 of 8 triangles: pos = 2 1 4 0 5 6 3 7
// (a reference that is no triangle id is skipped)
void tri_order(const uint32_t *refs, size_t n_refs, uint32_t n_tris, std::vector<uint32_t> &pos);

} // namespace yafgpu
