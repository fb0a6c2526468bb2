"""CPU: the name -> union index map of `merge` (host/merge_names.c) is correct
at any size and keeps insertion order -- past the 126 names at which the
reference's table starts to register names twice -- and ccq_merge_index finds
a name that one matrix holds twice."""
import numpy as np
import pytest

from ccphylo_amd import native


def phy_text(names):
    out = ["%10d\n" % len(names)]
    for i, nm in enumerate(names):
        out.append(nm + "".join("\t%d" % (i + j) for j in range(i)) + "\n")
    return "".join(out)


def test_namemap_insertion_order_at_any_size():
    lib = native.host_lib()
    M = lib.ccq_namemap_new()
    try:
        rng = np.random.default_rng(5)
        names = ["sample_%d" % k for k in rng.permutation(20000)[:5000]]
        for k, nm in enumerate(names):            # growth passes 64, 128 (the reference's table), 256 ...
            assert lib.ccq_namemap_add(M, nm.encode()) == k
            if k in (62, 63, 64, 126, 127, 128, 129, 255, 256, 4999):
                assert lib.ccq_namemap_n(M) == k + 1
                for j in rng.integers(0, k + 1, 20):
                    assert lib.ccq_namemap_add(M, names[j].encode()) == j
                assert lib.ccq_namemap_n(M) == k + 1
        assert [lib.ccq_namemap_name(M, k).decode() for k in (0, 127, 4999)] == [names[0], names[127], names[4999]]
        assert lib.ccq_namemap_name(M, 5000) is None and lib.ccq_namemap_name(M, -1) is None
        assert lib.ccq_namemap_add(M, b"") == 5000 and lib.ccq_namemap_add(M, b"") == 5000
    finally:
        lib.ccq_namemap_free(M)


def test_merge_indices_over_a_file(tmp_path):
    sets = [["a", "b", "c"], ["c", "x", "a", "y"], ["z"], ["y", "z", "b"]]
    p = tmp_path / "m.phy"
    p.write_text("".join(phy_text(s) for s in sets))
    names, idx = native.merge_indices(str(p))
    assert names == ["a", "b", "c", "x", "y", "z"]
    assert [list(v) for v in idx] == [[0, 1, 2], [2, 3, 0, 4], [5], [4, 5, 1]]


def test_merge_indices_past_the_reference_table(tmp_path):
    first = ["n%04d" % k for k in range(200)]
    later = ["n%04d" % k for k in range(1500)]
    p = tmp_path / "m.phy"
    p.write_text(phy_text(first) + phy_text(later[::-1]))
    names, idx = native.merge_indices(str(p))
    assert names == first + later[:199:-1]
    assert len(set(names)) == 1500 and sorted(idx[1]) == list(range(1500))
    assert list(idx[1][-200:]) == list(range(199, -1, -1))


def test_a_name_twice_in_one_matrix_is_found(tmp_path):
    p = tmp_path / "m.phy"
    p.write_text(phy_text(["a", "b"]) + phy_text(["b", "q", "c", "q"]))
    with pytest.raises(native.CcgError, match="matrix 2 .* rows 2 and 4"):
        native.merge_indices(str(p))
    # the same name in two matrices is the normal case
    p.write_text(phy_text(["a", "b"]) + phy_text(["b", "a"]))
    assert native.merge_indices(str(p))[0] == ["a", "b"]
