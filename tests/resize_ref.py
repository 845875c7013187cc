"""Float64 restatement of the latent resampler (include/sdmi.h "hires fix") for the tests: the tables of
sdmi_resize_weights applied with numpy, and torch's F.interpolate on the CPU, which defines them."""
import numpy as np
import torch
import torch.nn.functional as F

from stable_diffusion_burn_amd import resize_weights

MODES = ("nearest", "bilinear", "bicubic")            # sdmi mode 0, 1, 2
TORCH_MODES = ("nearest-exact", "bilinear", "bicubic")


def axis_matrix(in_size, out_size, mode, antialias):
    """(M [out, in] float64 with y = M x, max tap count) of one axis, from the C ABI's table"""
    first, count, taps = resize_weights(in_size, out_size, MODES[mode], bool(antialias))
    assert first.shape == count.shape == (out_size,) and taps.shape[0] == out_size
    assert (count >= 1).all() and (first >= 0).all() and (first + count <= in_size).all()
    m = np.zeros((out_size, in_size), np.float64)
    for o in range(out_size):
        assert not taps[o, count[o]:].any()            # unused slots are zero
        m[o, first[o]:first[o] + count[o]] = taps[o, :count[o]]
    return m, int(taps.shape[1])


def resize(x, out_h, out_w, mode, antialias=False):
    """x [n,c,h,w] -> (y [n,c,out_h,out_w] float64, S = sum |w_y| |w_x| |x| per output element, T_x, T_y): the horizontal pass, then the vertical one"""
    x = np.asarray(x, np.float64)
    mx, tx = axis_matrix(x.shape[3], out_w, mode, antialias)
    my, ty = axis_matrix(x.shape[2], out_h, mode, antialias)
    y = np.einsum("oh,nchp->ncop", my, np.einsum("pw,nchw->nchp", mx, x))
    s = np.einsum("oh,nchp->ncop", np.abs(my), np.einsum("pw,nchw->nchp", np.abs(mx), np.abs(x)))
    return y, s, tx, ty


def torch_resize(x, out_h, out_w, mode, antialias=False):
    """torch.nn.functional.interpolate on the CPU in float64: the definition"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    if mode == 0:
        return F.interpolate(t, size=(out_h, out_w), mode=TORCH_MODES[0]).numpy()
    return F.interpolate(t, size=(out_h, out_w), mode=TORCH_MODES[mode], align_corners=False, antialias=bool(antialias)).numpy()
