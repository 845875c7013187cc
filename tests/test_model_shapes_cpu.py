"""tests/model_shapes.py at full width, without a GPU: what tests/test_model_shapes_gpu.py promises of its two latent sizes, and the standard 64 x 64 model's
GEMM shapes as a cross-check of the rule (profiles/r01_gemm_shapes_b1.txt was recorded from them).  The rule itself is pinned against the engine's record on
the half-width model by the GPU module."""
import model_shapes as M
from oracle import sd_oracle as O

DIMS = O.Dims(320, 8, 768, 64, 64, 128)
SIZE_A, SIZE_B = (72, 88), (128, 128)


def test_shape_rule_at_full_width():
    a = M.unet_shapes(DIMS, *SIZE_A, 2)
    assert sorted({c.n * c.h * c.w for c in a.convs if c.k == 3 and c.stride == 1 and not c.ups}) == [198, 792, 3168, 12672]
    assert all((c.n * c.h * c.w) % 256 for c in a.convs)
    assert M.Conv(2, 2560, 9, 11, 1280, 3, 1, 0, "temb") in a.convs                      # K = 23040 at M = 99 n
    b = M.unet_shapes(DIMS, *SIZE_B, 2, levels=(0, 1))
    assert {c.n * c.h * c.w for c in b.convs} == {32768, 8192}
    assert M.Attention(2, 16384, 16384, 320, 8) in b.attentions and M.Attention(2, 16384, 77, 320, 8) in b.attentions
    assert M.Attention(1, 6336, 6336, 512, 1) in M.decoder_shapes(DIMS, *SIZE_A, 1).attentions
    std = M.unet_shapes(DIMS, 64, 64, 2).merge(M.decoder_shapes(DIMS, 64, 64, 1))
    for key in ("2,960,64,64,320,3,1,0", "2,2560,8,8,1280,3,1,0", "2,1280,16,16,1280,3,1,1", "2,320,64,64,320,3,2,0", "1,320,1,8192,960,1,1,0", "1,768,1,154,1280,1,1,0",
                "1,5120,1,512,1280,1,1,0", "1,512,128,128,512,3,1,1", "1,128,512,512,3,3,1,0", "1,4096,1,4096,512,1,1,0", "1,512,1,4096,4096,1,1,0"):
        assert key in std.gemm_keys(), key


def test_level_sizes_follow_the_stride_2_convolutions():
    assert M.level_sizes(72, 88) == [(72, 88), (36, 44), (18, 22), (9, 11)]
    assert M.level_sizes(8, 24) == [(8, 24), (4, 12), (2, 6), (1, 3)]
    assert M.level_sizes(128, 128)[:2] == [(128, 128), (64, 64)]


def test_levels_partition_the_shapes():
    """the items of the four levels together are the whole model's, for the UNet and the decoder"""
    for fn, n in ((M.unet_shapes, 2), (M.decoder_shapes, 1)):
        whole = fn(DIMS, *SIZE_A, n)
        parts = M.Shapes()
        for lv in range(4):
            parts.merge(fn(DIMS, *SIZE_A, n, levels=(lv,)))
        for f in M.Shapes.FIELDS:
            assert set(getattr(parts, f)) == set(getattr(whole, f)), f



def test_plane_rule_at_full_width():
    """M.arrives_as_planes on the layers named in its docstring"""
    s = M.unet_shapes(DIMS, *SIZE_A, 2).merge(M.decoder_shapes(DIMS, *SIZE_A, 1))
    fp32_in = [i for f in ("convs", "linears") for i in getattr(s, f) if not M.arrives_as_planes(i, DIMS)]
    assert {type(i).__name__ for i in fp32_in} == {"Conv", "Linear"}
    for i in fp32_in:
        if isinstance(i, M.Conv):
            assert i.cin == 4 or i.cout <= 4 or (i.k == 1 and i.cin == i.cout == 512 and i.n == 1), i
        else:
            assert i.rows == 1 or i.cin == 768, i
    assert all(M.arrives_as_planes(g, DIMS) for g in s.geglus)
