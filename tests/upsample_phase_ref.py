"""conv3x3(nearest_2x(x)) as four folded 2x2 phase convolutions -- the numpy statement of what the engine's phase launch computes (csrc/kernels.hpp,
ConvGemm::phases; csrc/k_gemm.hip fold_ups_phase_f64_kernel), shared by tests/test_upsample_phase_cpu.py and tests/test_upsample_phase_gpu.py.

Output pixel (2y + py, 2x + px): its three row taps ky = 0, 1, 2 read upsampled rows 2y + py - 1 + ky, i.e. source rows {y-1, y, y} for py = 0 and {y, y, y+1}
for py = 1; columns likewise with px.  The zero padding of the upsampled grid (rows -1 and 2H) is source row -1 / H, zero as well, so the border is exact.  With
R_0 = [[1,0,0],[0,1,1]], R_1 = [[1,1,0],[0,0,1]]:

    Wf[py][px][o][i][a][b] = sum_ky sum_kx R_py[a][ky] W[o][i][ky][kx] R_px[b][kx]
    y[n][o][2y+py][2x+px]  = bias[o] + sum_i sum_a sum_b Wf[py][px][o][i][a][b] x[n][i][y-1+py+a][x-1+px+b]        (zero outside)
"""
import numpy as np

R = np.array([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=np.float64)   # R[p][a][k]


def fold_weights(w):
    """w [O, I, 3, 3] -> Wf [4, O, I, 2, 2] in fp64, phase = py * 2 + px"""
    w = np.asarray(w, np.float64)
    out = np.empty((4,) + w.shape[:2] + (2, 2), np.float64)
    for py in range(2):
        for px in range(2):
            out[py * 2 + px] = np.einsum("ak,oikl,bl->oiab", R[py], w, R[px])
    return out


def packed_phase_image(w):
    """the engine's phase image [4][O][4 I] (I % 32 == 0): k = (channel slice * 4 + a * 2 + b) * 32 + channel within the slice"""
    wf = fold_weights(w)
    p, o, i = wf.shape[:3]
    return wf.reshape(p, o, i // 32, 32, 4).transpose(0, 1, 2, 4, 3).reshape(p, o, 4 * i)


def phase_conv(x, w, bias=None):
    """x [N, I, H, W], w [O, I, 3, 3] -> [N, O, 2H, 2W] by the phase form, fp64"""
    x = np.asarray(x, np.float64)
    wf = fold_weights(w)
    n, _, h, wd = x.shape
    o = wf.shape[1]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((n, o, 2 * h, 2 * wd), np.float64)
    for py in range(2):
        for px in range(2):
            acc = np.zeros((n, o, h, wd), np.float64)
            for a in range(2):
                for b in range(2):
                    # source pixel (y - 1 + py + a, x - 1 + px + b) = padded pixel (y + py + a, x + px + b)
                    acc += np.einsum("oi,nihw->nohw", wf[py * 2 + px, :, :, a, b], xp[:, :, py + a:py + a + h, px + b:px + b + wd])
            y[:, :, py::2, px::2] = acc
    if bias is not None:
        y += np.asarray(bias, np.float64)[None, :, None, None]
    return y


def phase_row(m, ph, hs, ws):
    """row m = (nb, y, x) of phase ph over the hs x ws source grid -> row of the [NB][2 hs][2 ws] output (csrc/kernels.hpp ups_phase_row)"""
    nb, rem = divmod(m, hs * ws)
    y, x = divmod(rem, ws)
    return (nb * 2 * hs + 2 * y + (ph >> 1)) * (2 * ws) + 2 * x + (ph & 1)
