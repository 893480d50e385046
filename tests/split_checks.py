"""Shared by the split-versus-whole stage tests (test_gpu_split_stage.py, test_gpu_slab2d_parts.py)."""
import numpy as np


def check_hll_switch(whole, split, nb):
    """`whole`, `split`: pion_gpu_get_hll_switch after the last step of the whole-stage and of the split run, all cells,
    [planes of the slab axis][...].  Equal on the on-grid planes -1 .. n of the slab axis, ghosts of the other axes
    included (the parts do not write the outermost ghost planes).  Against a vacuous pass, the whole-stage array must
    hold a set flag in the planes each part is the first to evaluate: the strips' [-1, nb-1) and [n-nb+1, n+1) and
    the interior part's [nb-1, n-nb+1)."""
    n = whole.shape[0] - 2 * nb
    regions = {"lower strip": (-1, nb - 1), "interior": (nb - 1, n - nb + 1), "upper strip": (n - nb + 1, n + 1)}
    counts = {k: int(np.count_nonzero(whole[nb + lo:nb + hi])) for k, (lo, hi) in regions.items()}
    print("set HLL flags of the whole-stage run:", counts)
    assert min(counts.values()) > 0, counts
    w, s = whole[nb - 1:nb + n + 1], split[nb - 1:nb + n + 1]
    assert np.array_equal(w, s), "%d flags differ, in planes %s" % ((w != s).sum(), sorted(set(np.nonzero(w != s)[0] - 1)))
