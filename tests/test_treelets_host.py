"""Host logic: the treelet layout of the flattened kd-tree (kdtree_build.h, TreeletLayout), the layout wf_trace walks.

Every node of the tree is reached from the root link by the same decoding the kernel uses (slot -> split and axis, the
children's links), and must carry the node's split and axis, or the leaf's reference range — inline or through the
escape array."""
import numpy as np
import pytest

from libyafaray_amd import scenes, interface

LEAF, ESCAPE, INDEX = 0x80000000, 0x40000000, 0x3FFFFFFF


def decode_leaf(link, leaves):
    assert link & LEAF
    if link & ESCAPE:
        first, np_ = leaves[link & INDEX]
        return int(first), int(np_)
    return link & 0xFFFFFF, (link >> 24) & 0x3F


def check_layout(nodes, words, leaves, root, inline_leaves):
    """walks nodes and links side by side; returns (interior nodes seen, leaves seen, escaped leaves seen)"""
    seen = [0, 0, 0]
    todo = [(0, int(root))]
    while todo:
        g, link = todo.pop()
        a, b = int(nodes[g, 0]), int(nodes[g, 1])
        if b & 3 == 3:
            first, np_ = decode_leaf(link, leaves)
            assert np_ == b >> 2 and (np_ == 0 or first == a), f"leaf {g}: link {link:#x}"
            if np_ == 0:
                assert link == LEAF, "an empty leaf is the empty link"
            elif not inline_leaves:
                assert link & ESCAPE
            seen[1] += 1
            seen[2] += bool(link & ESCAPE)
            continue
        assert not link & LEAF, f"interior node {g} reached through a leaf link"
        t, sl = link >> 2, link & 3
        assert sl < 3 and t < words.shape[0]
        w = words[t]
        hdr = int(w[3])
        assert int(w[sl]) == a and (hdr >> (2 * sl)) & 3 == b & 3, f"node {g}: split or axis"
        l_in = sl == 0 and (hdr >> 2) & 3 != 3
        r_in = sl == 0 and (hdr >> 4) & 3 != 3
        left = (link | 1) if l_in else int(w[6] if sl == 2 else w[4])
        right = (link | 2) if r_in else int(w[6] if sl == 0 else (w[5] if sl == 1 else w[7]))
        todo.append((g + 1, left))
        todo.append((b >> 2, right))
        seen[0] += 1
    return seen


def tree_of(verts):
    nodes, refs, bound, info = interface.build_kdtree(verts, threads=4)
    return nodes


@pytest.mark.parametrize("n_tris,seed", [(12, 1), (300, 2), (5000, 3), (40000, 4)])
@pytest.mark.parametrize("inline_leaves", [True, False])
def test_treelets_hold_the_tree(n_tris, seed, inline_leaves):
    nodes = tree_of(scenes.cornell_soup(n_tris, seed=seed)["verts"])
    words, leaves, root = interface.build_treelets(nodes, inline_leaves)
    interior, n_leaves, escaped = check_layout(nodes, words, leaves, root, inline_leaves)
    assert interior + n_leaves == nodes.shape[0], "every node is reached exactly once"
    # every treelet holds at least its root, so there are at most as many treelets as interior nodes, and at least a third
    assert (interior + 2) // 3 <= words.shape[0] <= interior
    n_nonempty = int(((nodes[:, 1] & 3) == 3).sum() - ((nodes[:, 1] == 3)).sum())
    assert escaped == (n_nonempty if not inline_leaves else leaves.shape[0])
    if inline_leaves:
        assert leaves.shape[0] == 0, "small trees fit inline"


def test_one_leaf_tree_and_stacked_triangles():
    # a tree that is one leaf: the root link is the leaf itself
    nodes = np.array([[0, 3 | (5 << 2)]], np.uint32)
    words, leaves, root = interface.build_treelets(nodes, True)
    assert words.shape[0] == 0 and decode_leaf(root, leaves) == (0, 5)
    # a leaf too large to go inline escapes, even with inline leaves
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    verts = np.concatenate([scenes.cornell_soup(200, seed=9)["verts"].reshape(-1, 9), np.repeat(tri, 100, axis=0)])
    nodes = tree_of(verts)
    words, leaves, root = interface.build_treelets(nodes, True)
    interior, n_leaves, escaped = check_layout(nodes, words, leaves, root, True)
    assert interior + n_leaves == nodes.shape[0]
    assert escaped >= 1 and escaped == leaves.shape[0]
