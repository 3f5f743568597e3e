"""The sparse stereo matcher without a GPU: the numpy twin (tests/stereo_ref.py) equals orc_stereo_match bit for bit on the
hand-made cases of tests/stereo_cases.py and on ORB's own keypoints, and every case reaches the exits and ties it was made
for - a case that no longer does fails here, not silently in tests/test_stereo_gpu.py."""
import numpy as np
import pytest

import stereo_cases
import stereo_ref
import util


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", stereo_cases.NAMES)
def test_twin_equals_oracle(orc, name):
    twin, uR, depth = stereo_cases.reference(name, orc)
    assert np.array_equal(bits(twin["uR"]), bits(uR)) and np.array_equal(bits(twin["depth"]), bits(depth))
    # what the twin adds is consistent with what both return
    acc = twin["reason"] == "accepted" if len(twin["reason"]) else np.zeros(0, bool)
    assert np.array_equal(twin["sad"] >= 0, acc) and np.array_equal(twin["uR"] >= 0, acc & ~twin["cut"])


@pytest.mark.parametrize("src", ["urban", "shifted"])
def test_twin_equals_oracle_on_orb_keypoints(orc, src):
    L, R = util.urban_pair(640, 240, 300, 60) if src == "urban" else util.shifted_pair(5, 640, 240, disparity=12)
    H, W = L.shape
    bf, fx = 386.1448, 718.856
    r = orc.stereo_frame(L, R, bf, fx)
    pL, pR = orc.build_pyramid(L), orc.build_pyramid(R)
    twin = stereo_ref.match(stereo_ref.split_pyramid(pL, W, H), stereo_ref.split_pyramid(pR, W, H), W, H,
                            r["kpL"], r["dL"], r["kpR"], r["dR"], bf, fx)
    assert len(r["kpL"]) > 300 and (r["depth"] > 0).sum() > 100
    assert np.array_equal(bits(twin["uR"]), bits(r["uR"])) and np.array_equal(bits(twin["depth"]), bits(r["depth"]))
    uR, depth, nv = orc.stereo_match(pL, pR, W, H, r["kpL"], r["dL"], r["kpR"], r["dR"], bf, fx)      # the wrapper itself
    assert np.array_equal(bits(uR), bits(r["uR"])) and np.array_equal(bits(depth), bits(r["depth"])) and nv == (r["depth"] > 0).sum()


@pytest.mark.parametrize("name", stereo_cases.NAMES)
def test_case_reaches_what_it_was_made_for(orc, name):
    c = stereo_cases.CASES[name]
    twin, _, _ = stereo_cases.reference(name, orc)
    got = stereo_ref.tally(twin)
    print(name, got)
    for key, least in c["need"].items():
        assert got.get(key, 0) >= least, (key, got)
    for i, j in c["partner"].items():
        assert twin["cand"][i] == j and twin["cand_dist"][i] <= 100, (i, j, twin["cand"][i])
    for i, j in c["missed"].items():
        assert twin["cand"][i] != j, (i, j)
    if c["sads"] is not None:
        assert sorted(twin["sad"][twin["sad"] >= 0].tolist()) == c["sads"]
    assert len(c["kpL"]) <= c["max_kp"] and len(c["kpR"]) <= c["max_kp"]


def test_cases_together_reach_every_exit(orc):
    total = {}
    for name in stereo_cases.NAMES:
        for k, v in stereo_ref.tally(stereo_cases.reference(name, orc)[0]).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert [k for k in stereo_cases.ALL_REACHED if total.get(k, 0) == 0] == []
    assert total.get("parabola", 0) == 0            # unreachable: the first strict minimum bounds |deltaR| by 0.5


def test_case_geometry_is_what_the_cases_claim():
    """borders_192: level 0 and an upper level have less than 5 bytes between width and the 64-byte pitch; the tall cases shift
    the 512 row buckets by 1, 2, 3; crowded_row fills one bucket with 512 keypoints; lanes >= 64 of one scan in `hamming`."""
    w, h, _ = stereo_ref.geometry(192, 128)
    tight = [l for l in range(8) if (w[l] + 63) // 64 * 64 - w[l] < 5]
    assert 0 in tight and len(tight) >= 2
    for H, shift in ((600, 1), (1100, 2), (2100, 3)):
        c = stereo_cases.CASES["tall_%d" % H]
        assert c["H"] == H and 256 <= (H >> shift) < 512
        rows = c["kpR"]["y"].astype(np.int64)
        assert rows.min() == 0 and rows.max() == H - 1
    c = stereo_cases.CASES["crowded_row"]
    assert len(c["kpR"]) == c["max_kp"] == 512 and set(c["kpR"]["y"].astype(np.int64)) == {70} and len(c["kpL"]) % 4
    for k in (8, 500):
        assert stereo_cases.CASES["small_ctx_%d" % k]["max_kp"] == k
    c = stereo_cases.CASES["hamming"]
    i = max(c["partner"])                           # the keypoint with three equal candidates
    rows = c["kpR"]["y"].astype(np.int64)
    row = int(c["kpL"]["y"][i])
    first = c["partner"][i]
    assert ((rows >= row - 9) & (rows < rows[first])).sum() >= 64


def test_binding_argument_checks(orc):
    c = stereo_cases.CASES["median_nd3"]
    pL, pR = orc.build_pyramid(c["L"]), orc.build_pyramid(c["R"])
    base = dict(pyrL=pL, pyrR=pR, **{k: c[k] for k in ("W", "H", "kpL", "dL", "kpR", "dR", "bf", "fx")})

    def args(**kw):
        return list(dict(base, **kw).values())

    orc.stereo_match(*args())
    with pytest.raises(ValueError):
        orc.stereo_match(*args(pyrL=pL[:-1]))
    with pytest.raises(ValueError):
        orc.stereo_match(*args(dL=c["dL"][:-1]))
    for field, bad in (("octave", 8), ("octave", -1), ("x", np.nan), ("y", np.inf), ("y", -1.0), ("y", float(c["H"])),
                       ("x", -c["W"] - 1.0), ("x", 2.0 * c["W"] + 1.0)):
        for side in ("kpL", "kpR"):
            k = c[side].copy()
            k[field][1] = bad
            with pytest.raises(ValueError):
                orc.stereo_match(*args(**{side: k}))
    k = c["kpL"].copy()
    k["x"][0] = -c["W"]                             # the limits themselves are legal
    k["y"][1] = np.nextafter(np.float32(c["H"]), np.float32(0))
    orc.stereo_match(*args(kpL=k))
    z = np.zeros(0, c["kpL"].dtype)
    uR, depth, nv = orc.stereo_match(*args(kpL=z, dL=np.zeros((0, 32), np.uint8)))
    assert len(uR) == 0 and nv == 0
