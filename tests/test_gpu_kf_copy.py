"""-m gpu: ptam_kf_copy — Level::operator= into an EXISTING keyframe (the pooled clone of the tracker -> mapmaker hand-off) against
ptam_kf_clone: every level's image, corners and row LUT byte for byte, the MakeKeyFrame_Rest tables made afterwards, and nothing of
what the destination held before shines through."""
import numpy as np
import pytest

from ptam_cg_amd import host, synth

pytestmark = pytest.mark.gpu


def _levels_equal(a, b):
    for l in range(4):
        la, lb = a.level(l), b.level(l)
        for f in ("im", "corners", "rowlut"):
            assert la[f].shape == lb[f].shape and la[f].tobytes() == lb[f].tobytes(), (l, f)


def _rest_equal(ra, rb):
    n = 0
    for l in range(4):
        for f in ("max_corners", "st_scores"):
            assert ra[l][f].shape == rb[l][f].shape and ra[l][f].tobytes() == rb[l][f].tobytes(), (l, f)
        n += len(ra[l]["max_corners"])
    return n


@pytest.mark.parametrize("size", [(163, 121), (640, 480)], ids=lambda s: "%dx%d" % s)
def test_copy_equals_clone(hip, size):
    w, h = size
    a, b = synth.make_frame_pair()
    a, b = np.ascontiguousarray(a[:h, :w]), np.ascontiguousarray(b[:h, :w])
    ctx = host.Context(lib=hip, size=size)
    src = host.KeyFrame(ctx).MakeKeyFrame_Lite(a)
    # the destination held ANOTHER image, its rest data and its in-plane corners
    dst = host.KeyFrame(ctx).MakeKeyFrame_Lite(np.ascontiguousarray(b[::-1]))
    rest_before = dst.MakeKeyFrame_Rest()
    dst.implane_corners(0)
    clone = src.clone()
    assert dst.copy_from(src) is dst
    _levels_equal(dst, clone)
    _levels_equal(dst, src)
    assert sum(len(src.level(l)["corners"]) for l in range(4)) > 50
    assert dst.implane_corners(0).tobytes() == clone.implane_corners(0).tobytes()
    rest_dst, rest_clone = dst.MakeKeyFrame_Rest(), clone.MakeKeyFrame_Rest()
    assert _rest_equal(rest_dst, rest_clone) > 20
    assert any(rest_dst[l]["max_corners"].tobytes() != rest_before[l]["max_corners"].tobytes() for l in range(4))
    # a source that HAS its rest data hands it over, as the clone does; the copy is reusable
    src.MakeKeyFrame_Lite(b)
    rest_src = src.MakeKeyFrame_Rest()
    dst.copy_from(src)
    _levels_equal(dst, src)
    n = host.C.c_int()
    for l in range(4):
        ctx._check(hip.kf_rest_info(ctx.h, dst.h, l, host.C.byref(n)), "kf_rest_info")
        mc, st = np.zeros((n.value, 2), np.int32), np.zeros(n.value)
        ctx._check(hip.kf_read_rest(ctx.h, dst.h, l, host._ptr(mc), host._ptr(st)), "kf_read_rest")
        assert mc.tobytes() == rest_src[l]["max_corners"].tobytes() and st.tobytes() == rest_src[l]["st_scores"].tobytes(), l
    _rest_equal(dst.MakeKeyFrame_Rest(), rest_src)
    for k in (src, dst, clone):
        k.close()
    ctx.close()


def test_refusals(hip):
    ctx, small = host.Context(lib=hip), host.Context(lib=hip, size=(163, 121))
    a, _ = synth.make_frame_pair()
    src = host.KeyFrame(ctx).MakeKeyFrame_Lite(a)
    other = host.KeyFrame(small).MakeKeyFrame_Lite(np.ascontiguousarray(a[:121, :163]))
    before = [other.level(l) for l in range(4)]
    assert hip.kf_copy(ctx.h, src.h, other.h) == -1          # another size
    assert hip.kf_copy(ctx.h, src.h, src.h) == -1            # onto itself
    assert hip.kf_copy(ctx.h, None, other.h) == -1 and hip.kf_copy(ctx.h, src.h, None) == -1 and hip.kf_copy(None, src.h, other.h) == -1
    for l in range(4):
        for f in ("im", "corners", "rowlut"):
            assert other.level(l)[f].tobytes() == before[l][f].tobytes()
    src.close()
    other.close()
    ctx.close()
    small.close()
