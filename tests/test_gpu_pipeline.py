"""Pass pipelining (yafaray_setPassPipelining / yafgpu_scene_set_pass_pipelining): consecutive renderPassDevice calls of independent passes
run their path work on two internal streams with a buffer set each.  What the caller sees must not change: every pass's planes bit for bit
those of the sequential render, the counters the same sums, and the caller's stream still orders its own work around the calls."""
import numpy as np
import pytest

from libyafaray_amd import Interface, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available()


def _setup(mode, transparent=False, **kw):
    sc = scenes.cornell_soup(600, seed=7, res=(96, 80), sigma=0.07)
    if transparent:     # every other soup triangle lets shadow rays through, filtered (as in test_gpu_parity.test_transparent_shadows)
        sc["materials"] = [dict(m) for m in sc["materials"]]
        sc["materials"].append({"type": "shinydiffusemat", "color": (0.3, 0.9, 0.4), "diffuse_reflect": 0.6, "transparency": 0.7, "transmit_filter": 0.8,
                                "specular_reflect": 0.2, "fresnel_effect": True, "IOR": 1.3})
        tm = np.array(sc["tri_mat"], np.int32)
        tm[np.arange(10, len(tm))[0::2]] = len(sc["materials"]) - 1
        sc["tri_mat"] = tm
    rd = scenes.render_settings(96, 80, 4, bounces=3, path_samples=1, integrator="pathtracing", **kw)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    yi.setPassPipelining(mode)
    yi.prepareRender()
    return yi


def _passes(yi, n, reuse_planes=False):
    import torch
    dev = torch.device("cuda", 0)
    W, H = yi.getRenderSize()
    counters = torch.zeros(8, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    outs = []
    planes = [torch.full((4, H, W, 5), 7.0, dtype=torch.float32, device=dev) for _ in range(1 if reuse_planes else n)]
    for k in range(n):
        p = planes[0 if reuse_planes else k]
        yi.renderPassDevice(p.data_ptr(), counters.data_ptr(), stream)
        if reuse_planes:
            outs.append(p.clone())      # on the caller's stream: must see pass k's film, not pass k + 1's
    torch.cuda.synchronize()
    if not reuse_planes:
        outs = planes
    return [o.cpu().numpy() for o in outs], counters.cpu().numpy()


@pytest.mark.parametrize("reuse_planes", [False, True])
def test_pipelined_passes_equal_sequential_passes(reuse_planes):
    seq, c_seq = _passes(_setup(0), 5, reuse_planes)
    pip, c_pip = _passes(_setup(1), 5, reuse_planes)
    assert np.array_equal(c_seq, c_pip), (c_seq, c_pip)
    assert c_seq[0] > 0 and c_seq[1] > 0
    for k, (a, b) in enumerate(zip(seq, pip)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"pass {k} differs"
    assert np.array_equal(seq[0].view(np.uint32), seq[4].view(np.uint32))      # (the same pass five times)


def test_transparent_shadows_in_pipelined_passes():
    """each buffer set has its own filter products of the shadow rays (transparent shadows); raydepth 0 keeps the passes free of recursion
    frames, so they are pipelined"""
    kw = dict(transparent=True, transpShad=True, shadowDepth=3, raydepth=0)
    seq, c_seq = _passes(_setup(0, **kw), 5)
    pip, c_pip = _passes(_setup(1, **kw), 5)
    assert np.array_equal(c_seq, c_pip), (c_seq, c_pip)
    assert c_seq[1] > 0      # rays_shadow
    for k, (a, b) in enumerate(zip(seq, pip)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"pass {k} differs"


@pytest.mark.parametrize("order", [((0, 1), (0, 2), (1, 2), (0, 1)), ((1, 2), (0, 2), (0, 1), (1, 2))], ids=["whole_first", "widening"])
def test_default_mode_pipelines_small_frames_and_a_frame_change_in_between_is_ordered(order):
    """mode -1 (by size) takes these small frames through the pipelined path; a change of the shard between two calls uploads new tile
    arrays on the caller's stream, which the internal streams must wait for.  The second order starts on half the frame and widens:
    each buffer set then grows while the other set's pass may be in flight"""
    import torch
    yi = _setup(-1)
    ref = _setup(0)
    dev = torch.device("cuda", 0)
    W, H = yi.getRenderSize()
    stream = torch.cuda.current_stream().cuda_stream
    for shards in order:
        got, want = [], []
        for it, dst in ((yi, got), (ref, want)):
            it.setShard(*shards)
            for k in range(3):
                p = torch.zeros((4, H, W, 5), dtype=torch.float32, device=dev)
                it.renderPassDevice(p.data_ptr(), 0, stream)
                dst.append(p)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"shard {shards}"


def test_a_failed_prepare_leaves_the_interface_unprepared():
    """prepareRender that refuses its parameters after an earlier success: nothing renders with the half-read set-up until a call
    succeeds again, and that one renders what the first did"""
    import torch
    from libyafaray_amd.interface import YafaRayError
    sc = scenes.cornell_soup(12, seed=7, res=(8, 8))
    rd = scenes.render_settings(8, 8, 2, bounces=2)
    yi = Interface()
    scenes.load_scene(yi, sc, rd)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    def one_pass():
        yi.prepareRender()
        assert yi.getRenderSize() == (8, 8)
        p = torch.zeros((4, 8, 8, 5), dtype=torch.float32, device=dev)
        yi.renderPassDevice(p.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        return p.cpu().numpy()

    first = one_pass()
    assert np.any(first != 0)
    scenes.set_render_params(yi, dict(rd, AA_passes=0))
    with pytest.raises(YafaRayError, match="AA_passes must be at least 1"):
        yi.prepareRender()
    with pytest.raises(YafaRayError, match="call prepareRender first"):
        yi.getRenderSize()
    p = torch.zeros((4, 8, 8, 5), dtype=torch.float32, device=dev)
    with pytest.raises(YafaRayError, match="call prepareRender first"):
        yi.renderPassDevice(p.data_ptr(), 0, stream)
    scenes.set_render_params(yi, dict(rd, AA_passes=1))
    again = one_pass()
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))


def test_accumulating_passes_add_up_in_call_order():
    """rp.accumulate passes (yafaray_render's later passes) add into the same planes: the float sums depend on the order, which is the
    caller's stream's — compared with the host-driven multi-pass render of the same settings, pipelining off"""
    kw = dict(AA_passes=3, AA_inc_samples=2, AA_threshold=0.0)
    a = _setup(1, **kw); b = _setup(0, **kw)
    a.render(); b.render()
    W, H = a.getRenderSize()
    fa, fb = a.getFilm(W, H), b.getFilm(W, H)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    sa, sb = a.getRenderStats(), b.getRenderStats()
    assert (sa.camera_samples, sa.rays_closest, sa.rays_shadow) == (sb.camera_samples, sb.rays_closest, sb.rays_shadow)
