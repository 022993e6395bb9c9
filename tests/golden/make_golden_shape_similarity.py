"""Writes tests/golden/ref_shape_similarity.npz: what the reference's ``spateo/tdr/morphometrics/shape_similarity.py`` gives on
the clouds of tests/_shape_cases.py (generated there from seeds: the golden holds reference outputs only).

The reference file imports only numpy and scipy and is loaded by path.  Per case and order (``<case>_<order>_``):
  ``vs``          (subspaces, 2) the reference's ``[cosine, dist]`` per kept subspace, in its voxel order;
  ``count``, ``voxel``   the rows per kept subspace, and its voxel id (the reference returns no ids: every subspace it returns is
                  matched, as a set of rows, to the voxel the table comparisons of _shape_cases.bin_points give - asserted);
  ``rank``, ``sv``  what ``scipy.linalg.lstsq`` reported inside ``subspace_surface_fitting`` (sv NaN-padded to p columns);
  ``dist_gelss``  the same ``dist`` with ``lapack_driver="gelss"`` in place of the default gelsd;
  ``e``, ``w``, ``e_gelss``, ``w_gelss``   ``calculate_eigenvector`` of both (cubic only).
Per pair ``score_<a>_<b>`` and ``score_gelss_<a>_<b>``.  A cloud of END_TO_END whose descriptors come within EDGE_MARGIN of a
bin edge of stage 4 stops the script: pick another seed in _shape_cases.py.

Run from the repository root where the reference checkout is readable (its path as the argument; default
``oracle.ref_stage.REFERENCE_TREE``):  python tests/golden/make_golden_shape_similarity.py [<spateo root>]"""
import importlib.util
import os
import sys

import numpy as np
import scipy
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _shape_cases as sc  # noqa: E402


def load_reference(root):
    path = os.path.join(root, "spateo", "tdr", "morphometrics", "shape_similarity.py")
    spec = importlib.util.spec_from_file_location("ref_shape_similarity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def descriptors(ref, pcs, n, order, driver):
    """The loop of the reference's ``model_eigenvector`` with ``order`` free and ``lstsq`` observed."""
    seen = []

    def lstsq(A, b):
        out = scipy.linalg.lstsq(A, b, lapack_driver=driver)
        seen.append((out[2], out[3]))
        return out

    ref.lstsq = lstsq
    try:
        subspaces = ref.rough_subspace(pcs=np.asarray(pcs).copy(), n=n)
        vs = []
        for sub in subspaces:
            surface = ref.subspace_surface_fitting(pcs=sub, order=order)
            g = np.mean(np.asarray(pcs).copy(), axis=0)
            vs.append([ref.cos_global_centroid_to_subspace(global_centroid=g, subspace_pcs=sub),
                       ref.dist_global_centroid_to_subspace(centroid=g, subspace_surface=surface)])
    finally:
        ref.lstsq = scipy.linalg.lstsq
    p = sc.P[order]
    sv = np.full((len(seen), p), np.nan)
    for i, (_, s) in enumerate(seen):
        sv[i, : len(s)] = s
    return subspaces, np.asarray(vs, dtype=np.float64), np.array([r for r, _ in seen], dtype=np.int32), sv


def main(root):
    ref = load_reference(root)
    out = {"scipy_version": np.array(scipy.__version__), "numpy_version": np.array(np.__version__)}
    vectors = {}
    for name, case in sc.CASES.items():
        pcs, n = case["pcs"], case["n"]
        pv, n_overlap = sc.bin_points(pcs, n)
        assert n_overlap == 0, (name, n_overlap)
        ids, counts, rows = sc.groups(pv)
        for order in case["orders"]:
            subspaces, vs, rank, sv = descriptors(ref, pcs, n, order, "gelsd")
            _, vs2, _, _ = descriptors(ref, pcs, n, order, "gelss")
            assert len(subspaces) == len(ids), (name, len(subspaces), len(ids))
            for sub, r in zip(subspaces, rows):   # the same rows (the reference sorts them by y)
                assert np.array_equal(sub[np.lexsort(sub.T)], pcs[r][np.lexsort(pcs[r].T)]), name
            assert np.array_equal(vs[:, 0], vs2[:, 0])
            key = f"{name}_{order}"
            out[f"{key}_vs"], out[f"{key}_count"], out[f"{key}_voxel"] = vs, counts, ids
            out[f"{key}_rank"], out[f"{key}_sv"], out[f"{key}_dist_gelss"] = rank, sv, vs2[:, 1]
            swap = np.abs(vs2[:, 1] - vs[:, 1]) / np.abs(vs[:, 1])
            marg = sc.marginal(sv)
            line = (f"{key}: {len(pcs)} points, n_subspace {n}, dropped {int((pv < 0).sum())}, {len(ids)} subspaces, counts "
                    f"{counts.min()}..{counts.max()}, ranks {rank.min()}..{rank.max()}, underdetermined {int((counts < sc.P[order]).sum())}, "
                    f"marginal {int(marg.sum())}, swap deviation max {swap.max():.2e} median {np.median(swap):.2e}")
            if order == "cubic":
                e, w = ref.calculate_eigenvector(vs, m=sc.M, s=sc.S)
                e2, w2 = ref.calculate_eigenvector(np.c_[vs2[:, 0], vs2[:, 1]], m=sc.M, s=sc.S)
                out[f"{key}_e"], out[f"{key}_w"], out[f"{key}_e_gelss"], out[f"{key}_w_gelss"] = e, w, e2, w2
                vectors[name] = ((e, w), (e2, w2))
                if name in sc.END_TO_END:
                    margin = min(sc.edge_margin(vs), sc.edge_margin(np.c_[vs2[:, 0], vs2[:, 1]]))
                    assert margin > sc.EDGE_MARGIN, (name, margin, "a descriptor sits on a bin edge: pick another seed")
                    line += f", nearest bin edge {margin:.2e}"
            print(line)
    for a, b in sc.PAIRS:
        for tag, k in (("score", 0), ("score_gelss", 1)):
            (e1, w1), (e2, w2) = vectors[a][k], vectors[b][k]
            w = np.max(np.c_[w1, w2], axis=1)
            out[f"{tag}_{a}_{b}"] = np.float64(round(np.sum(w * e1 * e2) / (np.linalg.norm(np.sqrt(w) * e1) * np.linalg.norm(np.sqrt(w) * e2)), 4))
        # the whole pairwise call once, as the users make it
        full = ref.pairwise_shape_similarity(sc.CASES[a]["pcs"], sc.CASES[b]["pcs"], n_subspace=sc.CASES[a]["n"], m=sc.M, s=sc.S) \
            if sc.CASES[a]["n"] == sc.CASES[b]["n"] else None
        assert np.isfinite(out[f"score_{a}_{b}"]) and np.isfinite(out[f"score_gelss_{a}_{b}"]), (a, b)
        assert full is None or full == out[f"score_{a}_{b}"], (a, b, full, out[f"score_{a}_{b}"])
        print(f"pair {a}-{b}: score {out[f'score_{a}_{b}']} (gelss {out[f'score_gelss_{a}_{b}']})")
    path = os.path.join(HERE, "ref_shape_similarity.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from oracle import ref_stage

        main(ref_stage.REFERENCE_TREE)
