"""tests/prune_ref.py against itself: the literal transcription of removeSlightlyLessTerribleFeatures (velo.h:282-326) and the
vectorised a[idx] form agree on crafted cases, and the properties the GPU prune is held to follow from either."""
import numpy as np
import pytest

import prune_ref as PR


def both(cam, rows, good):
    a, b = PR.prune_literal(cam, rows, good), PR.prune_vectorised(cam, rows, good)
    assert PR.same(a, b)
    return a


def test_permuted_has_depth():
    rng = np.random.default_rng(1)
    cam, rows = PR.make_camera(rng, 40, "all")
    assert sorted(cam[2].tolist()) == list(range(40)) and cam[2].tolist() != list(range(40))      # every slot once, not in keypoint order
    (ids, kps, has, cloud), r, kept = both(cam, rows, np.arange(0, 40, 3))
    assert has.tolist() == list(range(len(kept)))                       # jd++: the new cloud is in KEYPOINT order
    assert cloud.tobytes() == cam[3][cam[2][kept]].tobytes()


def test_shared_cloud_entry_kept_twice_grows_the_cloud():
    rng = np.random.default_rng(2)
    cam, rows = PR.make_camera(rng, 4, "shared")
    assert len(cam[3]) == 1
    (ids, kps, has, cloud), r, kept = both(cam, rows, [3, 0, 2, 1])
    assert has.tolist() == [0, 1, 2, 3] and len(cloud) == 4 and all(cloud[k].tobytes() == cam[3][0].tobytes() for k in range(4))


@pytest.mark.parametrize("n", [0, 1, 5, 33])
def test_all_none_one_duplicates_and_empty_camera(n):
    rng = np.random.default_rng(3 + n)
    cam, rows = PR.make_camera(rng, n, "mixed")
    for name, good in PR.keep_sets(rng, n).items():
        for rw in (rows, None):
            (ids, kps, has, cloud), r, kept = both(cam, rw, good)
            want = sorted(set(good.tolist()))
            assert kept.tolist() == want                                 # duplicates in good_matches count once
            if name == "all":
                assert ids.tobytes() == cam[0].tobytes() and kps.tobytes() == cam[1].tobytes()
            if name == "none":
                assert len(ids) == len(cloud) == 0


def test_a_kept_keypoints_depth_point_is_unchanged_and_order_is_kept():
    rng = np.random.default_rng(9)
    cam, rows = PR.make_camera(rng, 300, "mixed")
    good = PR.keep_sets(rng, 300)["half"]
    (ids, kps, has, cloud), r, kept = both(cam, rows, good)
    assert 0 < len(kept) < 300 and len(good) > len(kept)                 # the list holds duplicates
    for j, i in enumerate(kept):
        assert (has[j] == -1) == (cam[2][i] == -1)
        if has[j] != -1:
            assert cloud[has[j]].tobytes() == cam[3][cam[2][i]].tobytes()
        assert ids[j] == cam[0][i] and kps[j].tobytes() == cam[1][i].tobytes() and r[j].tobytes() == rows[i].tobytes()
    # the output is a subsequence of the input: strictly ascending old indices, every one once
    assert (np.diff(kept) > 0).all()
    wd = has[has != -1]
    assert wd.tolist() == list(range(len(wd)))
