"""The float64 restatement the GPU RMSD tests compare against (tests/_rmsd_util.py) reproduces the EXECUTED reference stored in
tests/golden/rmsd_golden.npz (made by tests/golden/make_rmsd_golden.py) within the reference's own float32 noise `ref_vs_f64`,
and the rank <-> ordering helper is itertools.permutations order.  No GPU, no kernel: passes with and without the feature."""
import itertools
import math

import numpy as np

from tests import _rmsd_util as RU
from tests._util import load_golden


def _split(a, sizes):
    return np.split(a, np.cumsum(sizes)[:-1])


def test_restatement_reproduces_the_three_spellings():
    G = load_golden("rmsd_golden.npz")
    f_rmsd, f_t, f_R = G["ref_vs_f64"]
    sizes = G["kabsch.sizes"]
    assert 2 == sizes.min() and sizes.max() == 64 and len(sizes) >= 40
    n_R = 0
    for k, (P, Q) in enumerate(zip(_split(G["kabsch.P"], sizes), _split(G["kabsch.Q"], sizes))):
        for name, (center, flip) in RU.SPELLINGS.items():
            s = G[f"kabsch.sigma_{center}"][k]
            assert np.allclose(s, RU.sigma_f64(P, Q, center), rtol=1e-9, atol=1e-12)
            R, t, rmsd = RU.kabsch_f64(P, Q, center, flip)
            if flip == "row" or RU.full_rank(s):
                assert abs(rmsd - float(G[f"kabsch.{name}.rmsd"][k])) <= f_rmsd * (1 + 1e-6) + 1e-12, (k, name)
            assert np.abs(t - G[f"kabsch.{name}.t"][k]).max() <= f_t * (1 + 1e-6) + 1e-12
            if RU.well_conditioned(s):
                n_R += 1
                assert np.abs(R - G[f"kabsch.{name}.R"][k]).max() <= f_R * (1 + 1e-6) + 1e-12, (k, name)
    assert n_R >= 90          # most of the 3 x 42 fits are compared in R
    # the reflection branch is taken, and the two fixes differ there (a noisy 4-atom cloud may prefer a reflection unmirrored)
    mirrored = G["kabsch.mirrored"].astype(bool)
    assert mirrored.sum() >= 12
    diff = np.abs(G["kabsch.torch.rmsd"] - G["kabsch.numpy_centroid.rmsd"])
    assert (diff[mirrored & (sizes >= 4)] > 1e-3).all() and (diff[~mirrored & (sizes >= 8)] < 1e-5).all()


def test_restatement_reproduces_the_search():
    G = load_golden("rmsd_golden.npz")
    sizes = G["search.sizes"]
    assert set(sizes.tolist()) == set(range(2, 9))
    orders = _split(G["search.order"], sizes)
    for k, (gen, orig) in enumerate(zip(_split(G["search.gen"], sizes), _split(G["search.orig"], sizes))):
        best, order, second = RU.search_f64(gen, orig)
        assert order == orders[k].tolist()
        assert abs(best - G["search.min_rmsd"][k]) <= G["ref_vs_f64"][0] * (1 + 1e-6)
        assert G["search.second_rmsd"][k] - G["search.min_rmsd"][k] >= RU.GAP * G["search.min_rmsd"][k]
        if math.isfinite(second):
            assert second - best >= 0.9 * RU.GAP * best


def test_rank_helper_is_itertools_order():
    for n in range(2, 8):
        perms = list(itertools.permutations(range(1, n)))
        assert len(perms) == math.factorial(n - 1)
        for rank, perm in enumerate(perms):
            order = [0] + list(perm)
            assert RU.rank_to_order(rank, n) == order
            assert RU.order_to_rank(order) == rank
        assert RU.all_orders(n).tolist() == [[0] + list(p) for p in perms]
    assert RU.rank_to_order(math.factorial(9) - 1, 10) == [0] + list(range(9, 0, -1))


def test_evaluate_golden_is_sorted_and_stable():
    G = load_golden("rmsd_golden.npz")
    r, idx = G["eval.ranked_rmsd"], G["eval.ranked_index"].tolist()
    assert (np.diff(r) >= 0).all()
    assert 1 not in idx and len(idx) == len(G["eval.sizes"]) - 1        # the one-atom graph is skipped
    assert idx.index(4) + 1 == idx.index(7)                            # the exact repeat keeps its list order
    assert G["eval.ranked_id"].tolist() == [G["eval.ids"][i] for i in idx]
