"""Float64 references, operands and bounds of the stem convolution's data gradient (conv_stem_dgrad_kernel, vpd_op_stem_dgrad) and
of the autograd path's custom loss (tests/test_stem_dgrad_ops_gpu.py, tests/test_autograd_gpu.py).  Nothing here touches the GPU
or the library: tests/test_autograd_cpu.py pins what these references rest on."""
import functools

import torch
import torch.nn.functional as F

from tests import opref as R

# (n, c_in, H, W)
STEM_DGRAD_CASES = {
    "min32_c5": (3, 5, 32, 32),          # smallest legal image: every pixel near a border; pixels no multiple of a 128-pixel tile
    "h32_w48_c3": (2, 3, 32, 48),        # H != W (24 column pairs: a partly filled 16-pair accumulator tile)
    "h64_w32_c8": (2, 8, 64, 32),        # full channel count
    "min32_c1": (1, 1, 32, 32),          # one channel, 15 padded slots of the 16 columns
    "w128_c5": (2, 5, 128, 128),         # the workload's row length
    # 40 x 16 x 1 = 640 tiles of 8 rows x 64 pairs on a grid of at most one block per compute unit (256): blocks walk 2-3 tiles --
    # the persistent loop, the next tile's register prefetch under the MFMAs, the re-stage behind the trailing barrier
    "tiles640_c5": (40, 5, 128, 128),
    # H % 8 != 0 (a partly filled row band), W % 4 != 0 (the 8-byte store path, an odd number of pairs), W > 128 (two column
    # tiles, the second partly filled); 40 x 5 x 2 = 400 tiles
    "h36_w162_c3": (40, 3, 36, 162),
}
STEM_DGRAD_K = 1024                      # 4 dz columns x 4 kernel rows x 64 channels: the longest sum of the launch


def stem_dgrad_ref(dz, w):
    """dx [n][c_in][H][W] (float64) of dz [n][64][H/2][W/2], w [64][c_in][7][7]"""
    return F.conv_transpose2d(dz.double(), w.double(), None, stride=2, padding=3, output_padding=1)


def stem_dgrad_autograd(dz, w):
    """the same as autograd of conv2d(x, w, stride 2, padding 3) sees it"""
    n, _, hz, wz = dz.shape
    x = torch.zeros(n, w.shape[1], 2 * hz, 2 * wz, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=2, padding=3).backward(dz.double())
    return x.grad


def stem_dgrad_parity(dz, w, skip_tap=None, skip_row=None, swap_pair=None):
    """The kernel's decomposition: for output row Y the kernel rows ky = Y + 1 (mod 2) with oy = (Y + 3 - ky) / 2; for the column
    pair X = 2 j + xpar the dz columns ox = j + dox, dox in -1..2, with kx = xpar + 3 - 2 dox (dropped outside 0..6).
    skip_tap = (ky, kx) with skip_row = Y: that tap left out on that output row; swap_pair = j: the two parities of that column
    pair exchanged (both: the alterations the bound has to reject)."""
    dz, w = dz.double(), w.double()
    n, co, hz, wz = dz.shape
    ci = w.shape[1]
    dx = torch.zeros(n, ci, 2 * hz, 2 * wz, dtype=torch.float64)
    dzp = F.pad(dz, (1, 2, 0, 0))                       # ox = -1 .. wz + 1 at index ox + 1
    for Y in range(2 * hz):
        for ky in range((Y + 1) % 2, 7, 2):
            oy = (Y + 3 - ky) // 2
            if oy < 0 or oy >= hz:
                continue
            row = dzp[:, :, oy, :]                      # [n][co][wz + 3]
            for xpar in range(2):
                for dox in range(-1, 3):
                    kx = xpar + 3 - 2 * dox
                    if kx < 0 or kx > 6 or (skip_tap == (ky, kx) and skip_row == Y):
                        continue
                    a = row[:, :, dox + 1:dox + 1 + wz]                       # dz[., ., oy, j + dox], j = 0 .. wz - 1
                    dx[:, :, Y, xpar::2] += torch.einsum("ncj,ck->nkj", a, w[:, :, ky, kx])
    if swap_pair is not None:
        j = swap_pair
        dx[:, :, :, [2 * j, 2 * j + 1]] = dx[:, :, :, [2 * j + 1, 2 * j]]
    return dx


def _seed(case, salt):
    n, ci, h, w = STEM_DGRAD_CASES[case]
    return salt * 100003 + n * 7919 + ci * 613 + h * 31 + w


@functools.lru_cache(maxsize=None)
def stem_dgrad_int_operands(case):
    """dz: sparse integers |k| <= 3 (exact in either element type); w = k / 8, |k| <= 8, independent per (co, ch, ky, kx): not
    symmetric in ky / kx nor across channels.  Every product is a multiple of 1/8 below 3 and a sum of 1024 of them stays below
    2^12: every partial sum is exact in fp32, in any order.  Returns (dz, w, reference), float64."""
    n, ci, h, w_ = STEM_DGRAD_CASES[case]
    g = torch.Generator().manual_seed(_seed(case, 1))
    dz = R._sparse_int((n, 64, h // 2, w_ // 2), 0.5, g, lo=3)
    w = torch.randint(-8, 9, (64, ci, 7, 7), generator=g).double() / 8.0
    return dz, w, stem_dgrad_ref(dz, w)


@functools.lru_cache(maxsize=None)
def stem_dgrad_randn_operands(case, name):
    """dz: randn rounded to the element type; w: fp32 randn (He-scaled), the reference uses its element-rounded value (what the
    kernel multiplies).  Returns (dz, w fp32, reference, bound): |got - ref| <= bound per element, the fp32 accumulator's error
    over at most 1024 exact products (the output is fp32: no element rounding)."""
    n, ci, h, w_ = STEM_DGRAD_CASES[case]
    g = torch.Generator().manual_seed(_seed(case, 2))
    dz = R.elem_round(torch.randn(n, 64, h // 2, w_ // 2, generator=g), name).double()
    w = (torch.randn(64, ci, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5).float()
    wq = R.elem_round(w, name).double()
    ref = stem_dgrad_ref(dz, wq)
    return dz, w, ref, stem_dgrad_bound(dz, wq)


def stem_dgrad_bound(dz, wq):
    return R.conv_gamma(stem_dgrad_ref(dz.abs(), wq.abs()), STEM_DGRAD_K)


# ---------------------------------------------------------------------------
# the loss the fused path cannot express: per-crop weighted cosine distillation
# ---------------------------------------------------------------------------
def crop_weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) + 0.5


def weighted_cosine_loss(emb, tgt, wts):
    """sum_i w_i (1 - cos(emb_i, t_i))"""
    return (wts * (1.0 - F.cosine_similarity(emb, tgt, dim=1))).sum()
