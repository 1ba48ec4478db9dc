"""The seeded pair list of the SfM fine-matching tests, shared by the CPU and the GPU file.

Five images in two size groups -- 96 x 128 (images 0, 1, 3) and 64 x 96 (images 2, 4) -- with ``scales`` other than one except on
image 0, whose unit scale carries the half-cell ties; seven pairs with 300 rows in all, two of them between the size groups, one with
a single row.  x runs from 10 px left of every image to 10 px right of it (both sides of the clip limits 0 and W - 2, and the wrap of
a clipped x into the next row of cells); y from 10 px above the image to 10 px below it where the clipped y (H - 2) still rounds to a
cell at least two rows above the grid's last (images 1, 2 and 4, whose h factor is 1.25 or more: both sides of the clip limit again),
and to the last y that does so elsewhere.  No row of the list rounds outside its grid: the tests that want such a row plant it.
"""
import numpy as np
import torch

SIZES = ((96, 128), (96, 128), (64, 96), (96, 128), (64, 96))
SCALES = ((1.0, 1.0), (1.25, 0.8), (1.5, 0.9), (1.1, 1.2), (1.3, 1.0))             # the reference's (h factor, w factor) per image
PAIRS = ((0, 1, 60), (0, 3, 50), (1, 3, 45), (1, 2, 40), (2, 4, 45), (3, 0, 1), (4, 1, 59))      # (left, right, rows)
GROUP = (0, 0, 1, 0, 1)
N_TIES = 12


def _keypoints(g, n, image):
    H, W = SIZES[image]
    cell = 8.0 * SCALES[image][0]
    y_top = H + 10.0 if (H - 2) / cell <= H // 8 - 2 else cell * (H // 8 - 2.5)      # the clipped y itself stays two rows above the last
    x = torch.rand(n, generator=g, dtype=torch.float64) * (W + 20) - 10
    y = torch.rand(n, generator=g, dtype=torch.float64) * (y_top + 10) - 10
    return torch.stack([x, y], 1)


def pair_list(dtype=torch.float64, seed=5):
    """-> host tensors ``mkpts0_c``, ``mkpts1_c [300, 2]`` (``dtype``), ``row_left``, ``row_right [300]``, ``pair_left``, ``pair_right
    [7]``, ``pair_offsets [8]``, ``mkpts0_idx [300]``"""
    g = torch.Generator().manual_seed(seed)
    k0, k1, left, right = [], [], [], []
    for l, r, n in PAIRS:
        a, b = _keypoints(g, n, l), _keypoints(g, n, r)
        if (l, r) == (0, 1):                       # ties: x = 8 k + 4 lies on a cell's half at unit scale -> round half to even
            a[:N_TIES, 0] = 8.0 * torch.arange(N_TIES) + 4.0
        k0.append(a)
        k1.append(b)
        left += [l] * n
        right += [r] * n
    counts = [n for _, _, n in PAIRS]
    return {"mkpts0_c": torch.cat(k0).to(dtype), "mkpts1_c": torch.cat(k1).to(dtype), "row_left": torch.tensor(left), "row_right": torch.tensor(right),
            "pair_left": torch.tensor([p[0] for p in PAIRS]), "pair_right": torch.tensor([p[1] for p in PAIRS]),
            "pair_offsets": torch.tensor(np.concatenate([[0], np.cumsum(counts)])), "mkpts0_idx": torch.arange(sum(counts))}


def bucket_keys(pairs):
    """(size group of the left image) * 2 + (size group of the right image) per row"""
    grp = torch.tensor(GROUP)
    return (grp[pairs["row_left"]] * 2 + grp[pairs["row_right"]]).numpy()


def images(seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(1, 1, H, W, generator=g) for H, W in SIZES]


def scales():
    return torch.tensor(SCALES, dtype=torch.float32)
