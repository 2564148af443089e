"""The device-resident sliding-window scan map (velo_map_*) on the GPU.  The yardstick is always a SECOND context fed
velo_set_target(the restatement's cloud, tests/scan_map_ref.py), never the new call: a loaded map must be that target byte for byte --
cloud, ring offsets, and through them every registration result."""
import ctypes as C

import numpy as np
import pytest

import scan_map_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu

EYE = np.eye(4)
RING_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@pytest.fixture(scope="module")
def drive():
    d = synth.drive(7, n_beams=16, n_azimuth=128)
    d["frames"] = [(np.ascontiguousarray(np.asarray(x, np.float32)[:, :3]), np.asarray(o, np.int32)) for x, o in d["frames"]]
    Cm = synth.VELO_TO_CAM.astype(np.float64)
    d["poses_cam"] = [Cm @ P @ np.linalg.inv(Cm) for P in d["poses_velo"]]        # the drive's own chain, camera frame
    return d


@pytest.fixture(scope="module")
def ctxs():
    cs = [api.Context(0, icp_skip=2) for _ in range(4)]
    yield cs
    for c in cs:
        c.close()


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    T = np.eye(4)
    T[i, i], T[i, j], T[j, i], T[j, j] = c, -s, s, c
    return T


def shift(x, y, z):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def rigid_inverse(P):
    Q = np.eye(4)
    Q[:3, :3] = P[:3, :3].T
    Q[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return Q


def crafted(sizes, seed):
    """rings of the given sizes: noisy circles of a metre's height step, so every ring is a usable target ring"""
    rng = np.random.default_rng(seed)
    pts, off = [], [0]
    for r, n in enumerate(sizes):
        a = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = 6.0 + 0.5 * r + rng.normal(size=n) * 0.02
        pts.append(np.stack([rad * np.cos(a), np.full(n, -1.5 + 0.2 * r) + rng.normal(size=n) * 0.01, rad * np.sin(a)], axis=1))
        off.append(off[-1] + n)
    return np.concatenate(pts).astype(np.float32), np.asarray(off, np.int32)


def put(c, m, ref, frame, xyz, off, pose):
    """the scan enters the map from the context's source side, and the restatement"""
    c.set_source(xyz, off)
    gone = m.insert(c, False, frame, pose)
    assert gone == ref.insert(frame, xyz, off, pose)
    return gone


def same_floats(a, b):
    """byte-equal where finite; the np.isfinite masks equal; NaN payloads are not compared"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    fa, fb = np.isfinite(a), np.isfinite(b)
    return a.shape == b.shape and np.array_equal(fa, fb) and a[fa].tobytes() == b[fb].tobytes() and \
        np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fa & ~np.isnan(a)], b[~fb & ~np.isnan(b)])


def check_load(m, ref, c, yard, ref_inv, exact=True):
    """load into c; the restatement's cloud through velo_set_target into yard; both targets are the restatement's"""
    m.load(c, ref_inv)
    cloud, off = ref.materialise(ref_inv)
    yard.set_target(cloud, off)
    got = c.cloud(True)
    if exact:
        assert got.tobytes() == cloud.tobytes() == yard.cloud(True).tobytes()
    else:
        assert same_floats(got, cloud) and same_floats(got, yard.cloud(True))
    assert np.array_equal(c.ring_offsets(True), off) and np.array_equal(yard.ring_offsets(True), off)
    return cloud, off


def check_state(m, ref):
    """velo_map_frames, velo_map_info and velo_map_get_scan equal the restatement"""
    assert m.frames() == ref.frames()
    info, want = m.info(), ref.info()
    for k, v in want.items():
        assert info[k] == v, (k, info, want)
    for frame, xyz, off, pose in ref.scans:
        gx, go, gp = m.get_scan(frame)
        assert gx.tobytes() == xyz.tobytes() and np.array_equal(go, off) and gp.tobytes() == pose.tobytes()


def summary_bytes(s):
    rows = [(v.termination, v.lm_iterations, v.evaluations, v.n_icp_valid, v.n_visual_blocks, v.initial_cost, v.final_cost)
            for v in (s.solves[k] for k in range(s.n_solves))]
    return np.asarray([(s.n_solves, s.n_assoc_rounds, s.n_queries, s.n_target, 0, 0, 0)] + rows, dtype=np.float64).tobytes()


def register(c, x0):
    x, T, s = c.frame_to_frame(x0)
    return x.tobytes() + T.tobytes() + summary_bytes(s)


# ---- the loaded cloud ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", RING_SIZES)
def test_one_scan_of_one_ring_size(ctxs, size):
    m, ref = api.ScanMap(0, 4, 1 << 20), R.ScanMapRef(4, 1 << 20)
    xyz, off = crafted([size, size, size], size)
    put(ctxs[0], m, ref, 5, xyz, off, rot(1, 0.3) @ shift(1.0, 0.0, 2.0))
    check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(rot(0, -0.1) @ shift(0.5, 0.1, 0.0)))
    check_state(m, ref)


def test_all_ring_sizes_mixed_in_one_map(ctxs):
    m, ref = api.ScanMap(0, 16, 1 << 20), R.ScanMapRef(16, 1 << 20)
    for k, size in enumerate(RING_SIZES):
        xyz, off = crafted([size, RING_SIZES[(k + 3) % 10], size], 100 + k)
        put(ctxs[0], m, ref, k, xyz, off, rot(k % 3, 0.05 * k) @ shift(0.7 * k, 0.0, 0.1 * k))
    check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(ref.scans[-1][3]))
    check_state(m, ref)


@pytest.mark.parametrize("n_scans", (1, 2, 17, 65))
def test_window_lengths(ctxs, drive, n_scans):
    """65 scans of 8 rings: the unit table is longer than a wave"""
    m, ref = api.ScanMap(0, 80, 1 << 21), R.ScanMapRef(80, 1 << 21)
    for k in range(n_scans):
        if n_scans == 65:
            xyz, off = crafted([37 + (k % 5)] * 8, 300 + k)
        else:
            xyz, off = drive["frames"][k % 7]
        put(ctxs[0], m, ref, k, xyz, off, rot(1, 0.01 * k) @ shift(0.0, 0.0, 0.9 * k))
    _, off = check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(ref.scans[-1][3]))
    if n_scans == 65:
        assert len(off) - 1 == 65 * 8
    check_state(m, ref)


POSES = {"identity": EYE, "about x": rot(0, 0.7), "about y": rot(1, -1.9), "about z": rot(2, 2.6), "1000 m": shift(1000.0, -3.0, 1000.0)}


@pytest.mark.parametrize("name", list(POSES))
def test_poses(ctxs, drive, name):
    m, ref = api.ScanMap(0, 4, 1 << 20), R.ScanMapRef(4, 1 << 20)
    put(ctxs[0], m, ref, 0, *drive["frames"][0], POSES[name])
    put(ctxs[0], m, ref, 1, *drive["frames"][1], POSES[name] @ shift(0.0, 0.0, 1.0))
    cloud, _ = check_load(m, ref, ctxs[0], ctxs[1], EYE)
    if name == "identity":
        assert cloud[:len(drive["frames"][0][0])].tobytes() == (drive["frames"][0][0] + np.float32(0.0)).tobytes()
    if name == "1000 m":                                 # float rounding bites: floats below 2048 are 2^-13 apart at most
        back = cloud[:len(drive["frames"][0][0])].astype(np.float64) - POSES[name][:3, 3]
        assert 1e-6 < np.abs(back - drive["frames"][0][0]).max() <= 2.0 ** -14
    check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(POSES[name]))


def test_the_drives_own_chain(ctxs, drive):
    m, ref = api.ScanMap(0, 8, 1 << 20), R.ScanMapRef(8, 1 << 20)
    for k in range(7):
        put(ctxs[0], m, ref, k, *drive["frames"][k], drive["poses_cam"][k])
    for k in (6, 0, 3):
        check_load(m, ref, ctxs[0], ctxs[1], np.linalg.inv(drive["poses_cam"][k]))
    check_state(m, ref)


def test_negative_zero_comes_out_positive(ctxs):
    xyz, off = crafted([70, 70], 9)
    xyz[3] = [-0.0, -0.0, -0.0]
    xyz[80, 1] = -0.0
    m, ref = api.ScanMap(0, 2, 4096), R.ScanMapRef(2, 4096)
    put(ctxs[0], m, ref, 0, xyz, off, EYE)
    assert np.signbit(m.get_scan(0)[0][3]).all()          # stored as it came
    cloud, _ = check_load(m, ref, ctxs[0], ctxs[1], EYE)
    assert not np.signbit(ctxs[0].cloud(True)[3]).any() and not np.signbit(cloud[80, 1])


def test_non_finite_points(ctxs):
    xyz, off = crafted([90, 130, 64], 12)
    xyz[5, 0], xyz[100, 1], xyz[101] = np.nan, np.inf, [-np.inf, np.nan, 1.0]
    m, ref = api.ScanMap(0, 2, 4096), R.ScanMapRef(2, 4096)
    put(ctxs[0], m, ref, 0, xyz, off, rot(1, 0.4) @ shift(1.0, 2.0, 3.0))
    cloud, _ = check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(shift(0.5, 0.0, 0.0)), exact=False)
    fin = np.isfinite(cloud).all(axis=1)
    assert (~fin).sum() == 3 and fin.sum() == len(xyz) - 3


# ---- where a scan comes from -----------------------------------------------------------------------------------------------------------
def test_insert_from_source_promoted_target_and_velodyne(ctxs, drive):
    c, y = ctxs[0], ctxs[1]
    m, ref = api.ScanMap(0, 8, 1 << 20), R.ScanMapRef(8, 1 << 20)
    put(c, m, ref, 0, *drive["frames"][0], drive["poses_cam"][0])
    # a promoted target
    c.set_source(*drive["frames"][1])
    c.source_to_target()
    assert m.insert(c, True, 1, drive["poses_cam"][1]) == 0
    ref.insert(1, *drive["frames"][1], drive["poses_cam"][1])
    # a target that was set
    c.set_target(*drive["frames"][2])
    assert m.insert(c, True, 2, drive["poses_cam"][2]) == 0
    ref.insert(2, *drive["frames"][2], drive["poses_cam"][2])
    # raw Velodyne records, segmented on the device: the context says what it holds
    rec = synth.hdl64_scan(synth.Scene(0), synth.pose_matrix(**synth.TRUE_MOTION), noise_seed=77, n_beams=16, n_azimuth=128)
    rec = np.concatenate([rec, np.zeros((len(rec), 1))], axis=1).astype(np.float32)
    for as_target, frame in ((False, 3), (True, 4)):
        c.set_scan_velodyne(as_target, rec, synth.VELO_TO_CAM)
        xyz, off = c.cloud(as_target), c.ring_offsets(as_target)
        assert m.insert(c, as_target, frame, drive["poses_cam"][3]) == 0
        ref.insert(frame, xyz, off, drive["poses_cam"][3])
    check_state(m, ref)
    check_load(m, ref, c, y, np.linalg.inv(drive["poses_cam"][3]))


def test_source_with_empty_rings_is_accepted(ctxs):
    xyz, off = crafted([50, 60, 70], 3)
    off = np.asarray([0, 0, 50, 50, 50, 110, 180, 180], np.int32)
    m, ref = api.ScanMap(0, 2, 4096), R.ScanMapRef(2, 4096)
    put(ctxs[0], m, ref, 0, xyz, off, EYE)
    assert m.info()["rings"] == 3 and m.get_scan(0)[1].tolist() == [0, 50, 110, 180]
    check_load(m, ref, ctxs[0], ctxs[1], rigid_inverse(shift(0.0, 0.0, 1.0)))


def test_what_the_scan_cache_refuses_is_refused(drive):
    c = api.Context(0, icp_skip=2)
    m = api.ScanMap(0, 4, 1 << 20)
    cache = api.ScanCache(0, 4)
    for of_target in (False, True):                       # nothing on that side
        with pytest.raises(api.VeloError, match="holds no"):
            cache.store(1, c, of_target)
        with pytest.raises(api.VeloError, match="holds no"):
            m.insert(c, of_target, 1, EYE)
    xyz, off = drive["frames"][0]
    half = int(off[8])
    c.set_target_part(xyz[half:], off[8:] - half, 8, half)     # a target shard is not a whole scan
    with pytest.raises(api.VeloError, match="shard"):
        cache.store(1, c, True)
    with pytest.raises(api.VeloError, match="shard"):
        m.insert(c, True, 1, EYE)
    none = np.zeros(3, np.int32)                                           # a scan with no point at all: two empty rings
    c._check(c._lib.velo_set_source(c.handle, None, 12, C.c_void_p(none.ctypes.data), 2, 0))
    with pytest.raises(api.VeloError, match="no point"):
        m.insert(c, False, 1, EYE)
    c.set_source(xyz, off)
    bad = EYE.copy()
    bad[1, 3] = np.nan
    with pytest.raises(api.VeloError, match="finite"):
        m.insert(c, False, 1, bad)
    assert m.frames() == [] and m.info()["points"] == 0
    c.close()


# ---- eviction and the arena ------------------------------------------------------------------------------------------------------------
def test_eviction_drop_clear_and_arena_growth(ctxs, drive):
    c, y = ctxs[0], ctxs[1]
    m, ref = api.ScanMap(0, 3, 1 << 20), R.ScanMapRef(3, 1 << 20)
    first = m.info()
    assert first["arena_points"] * 16 == 4096 and first["arena_growths"] == 0           # the arena starts at 4 KB
    for k in range(6):                                    # max_scans = 3, 6 inserts: the oldest go
        assert put(c, m, ref, k, *drive["frames"][k], drive["poses_cam"][k]) == (0 if k < 3 else 1)
        check_state(m, ref)
        check_load(m, ref, c, y, np.linalg.inv(drive["poses_cam"][k]))
    assert m.frames() == [3, 4, 5]
    grown = m.info()
    assert grown["arena_growths"] >= 1 and grown["arena_points"] >= grown["points"] and grown["evictions"] == 3
    # drop from the middle, then re-insert: the window order is insertion order, the freed block is taken again
    m.drop(4)
    ref.drop(4)
    check_state(m, ref)
    check_load(m, ref, c, y, np.linalg.inv(drive["poses_cam"][5]))
    put(c, m, ref, 4, *drive["frames"][4], drive["poses_cam"][4])
    assert m.frames() == [3, 5, 4]
    check_state(m, ref)
    check_load(m, ref, c, y, np.linalg.inv(drive["poses_cam"][5]))
    steady = m.info()["arena_growths"]
    for k in (6, 0, 1, 2):                                # a full window in the steady state: no growth any more
        put(c, m, ref, 10 + k, *drive["frames"][k], drive["poses_cam"][k])
    assert m.info()["arena_growths"] == steady
    check_state(m, ref)
    check_load(m, ref, c, y, EYE)
    m.clear()
    ref.clear()
    check_state(m, ref)
    assert m.info()["scans"] == 0 and m.info()["points"] == 0
    put(c, m, ref, 0, *drive["frames"][0], EYE)           # and it fills again
    check_state(m, ref)
    check_load(m, ref, c, y, EYE)


def test_point_budget_evicts_two_scans_at_once(ctxs):
    c, y = ctxs[0], ctxs[1]
    m, ref = api.ScanMap(0, 10, 1000), R.ScanMapRef(10, 1000)
    for k in range(3):
        assert put(c, m, ref, k, *crafted([100, 150], 40 + k), shift(0.0, 0.0, 1.0 * k)) == 0
        check_state(m, ref)
    assert put(c, m, ref, 3, *crafted([300, 300], 44), shift(0.0, 0.0, 3.0)) == 2       # 750 + 600, 500 + 600 > 1000; 250 + 600 fits
    assert m.frames() == [2, 3] and m.info()["points"] == 850
    check_state(m, ref)
    check_load(m, ref, c, y, rigid_inverse(shift(0.0, 0.0, 3.0)))
    # a scan larger than the budget is refused with nothing evicted
    c.set_source(*crafted([600, 401], 45))
    with pytest.raises(api.VeloError, match="does not fit"):
        m.insert(c, False, 9, EYE)
    assert ref.insert(9, *crafted([600, 401], 45), EYE) is None
    check_state(m, ref)
    assert put(c, m, ref, 9, *crafted([600, 400], 46), EYE) == 2
    check_state(m, ref)
    check_load(m, ref, c, y, EYE)


# ---- poses -----------------------------------------------------------------------------------------------------------------------------
def test_set_pose_and_two_reference_frames(ctxs, drive):
    m, ref = api.ScanMap(0, 4, 1 << 20), R.ScanMapRef(4, 1 << 20)
    for k in range(3):
        put(ctxs[0], m, ref, k, *drive["frames"][k], drive["poses_cam"][k])
    before, _ = check_load(m, ref, ctxs[0], ctxs[1], np.linalg.inv(drive["poses_cam"][2]))
    fixed = drive["poses_cam"][1] @ rot(1, 0.02) @ shift(0.05, 0.0, -0.1)                # a loop closure corrects frame 1
    m.set_pose(1, fixed)
    ref.set_pose(1, fixed)
    check_state(m, ref)
    after, _ = check_load(m, ref, ctxs[0], ctxs[1], np.linalg.inv(drive["poses_cam"][2]))
    n0, n1 = len(drive["frames"][0][0]), len(drive["frames"][1][0])
    assert before[:n0].tobytes() == after[:n0].tobytes() and before[n0:n0 + n1].tobytes() != after[n0:n0 + n1].tobytes()
    # one map, two contexts, two reference frames: both right, and both stay right
    a, _ = check_load(m, ref, ctxs[0], ctxs[1], np.linalg.inv(drive["poses_cam"][0]))
    b, _ = check_load(m, ref, ctxs[2], ctxs[3], np.linalg.inv(drive["poses_cam"][2]))
    assert ctxs[0].cloud(True).tobytes() == a.tobytes() and ctxs[2].cloud(True).tobytes() == b.tobytes() and a.tobytes() != b.tobytes()


# ---- registration ----------------------------------------------------------------------------------------------------------------------
def test_registration_against_a_loaded_map_is_bit_equal(ctxs, drive):
    a, y, b, z = ctxs
    m, ref = api.ScanMap(0, 4, 1 << 20), R.ScanMapRef(4, 1 << 20)
    for k in range(3):
        put(a, m, ref, k, *drive["frames"][k], drive["poses_cam"][k])
    ref_inv = np.linalg.inv(drive["poses_cam"][2])
    check_load(m, ref, a, y, ref_inv)
    x0 = np.asarray(drive["x_true"][2]) * 0.9
    for c in (a, y):
        c.set_source(*drive["frames"][3])
    assert register(a, x0) == register(y, x0)
    # the same through the batch entry, and on contexts that took the targets by reference
    b.share_target(a)
    z.share_target(y)
    for c in (b, z):
        c.set_source(*drive["frames"][4])
    assert register(b, x0) == register(z, x0)
    for c in (a, y):
        c.set_source(*drive["frames"][3])
    xa, Ta, Sa = api.frame_to_frame_batch([a, b], [x0, x0])
    xy, Ty, Sy = api.frame_to_frame_batch([y, z], [x0, x0])
    assert xa.tobytes() == xy.tobytes() and Ta.tobytes() == Ty.tobytes() and [summary_bytes(s) for s in Sa] == [summary_bytes(s) for s in Sy]
    for c in (b, z):                                      # let go of the shared targets: the next test loads into a and y again
        c.set_target(*drive["frames"][0])


def walk(c, frames, x_first, window, map_step):
    """6 frames, a window of 3: every frame is registered against the map in the newest pose's frame with the constant-velocity guess
    (the previous solution) and enters the map with its solved pose.  map_step(k, pose) -> loads the target / stores the scan."""
    poses, x = [EYE.copy()], np.asarray(x_first, np.float64)
    for k, (xyz, off) in enumerate(frames):
        c.set_source(xyz, off)
        if k > 0:
            map_step("load", k, rigid_inverse(poses[-1]))
            x, T, _ = c.frame_to_frame(x)
            poses.append(poses[-1] @ T)
        map_step("insert", k, poses[-1])
    return np.stack(poses)


def test_the_loop_equals_the_uploaded_walk(ctxs, drive):
    a, y = ctxs[0], ctxs[1]
    frames = drive["frames"][:6]
    m, ref_a, ref_y = api.ScanMap(0, 3, 1 << 20), R.ScanMapRef(3, 1 << 20), R.ScanMapRef(3, 1 << 20)

    def resident(what, k, P):
        if what == "load":
            m.load(a, P)
        else:
            assert m.insert(a, False, k, P) == ref_a.insert(k, *frames[k], P)

    def uploaded(what, k, P):
        if what == "load":
            y.set_target(*ref_y.materialise(P))
        else:
            ref_y.insert(k, *frames[k], P)

    pa = walk(a, frames, drive["x_true"][0], 3, resident)
    py = walk(y, frames, drive["x_true"][0], 3, uploaded)
    assert pa.tobytes() == py.tobytes()
    assert m.frames() == [3, 4, 5]
    check_state(m, ref_a)
    moved = np.linalg.norm(pa[-1][:3, 3])
    assert 2.0 < moved < 8.0                              # five steps of 0.6 .. 1.4 m: the registrations follow the drive


# ---- batch -----------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_single_loads(ctxs, drive):
    a, b, c, y = ctxs
    m1, r1 = api.ScanMap(0, 8, 1 << 20), R.ScanMapRef(8, 1 << 20)
    m2, r2 = api.ScanMap(0, 8, 1 << 20), R.ScanMapRef(8, 1 << 20)
    for k in range(4):                                    # 4 drive scans of 16 rings
        put(a, m1, r1, k, *drive["frames"][k], drive["poses_cam"][k])
    for k in range(2):                                    # 2 scans of 5 rings: the drive's, cut short
        xyz, off = drive["frames"][5 + k]
        put(b, m2, r2, k, xyz[:off[5]], off[:6], shift(0.0, 0.0, 0.8 * k))
    invs = [np.linalg.inv(drive["poses_cam"][3]), rigid_inverse(shift(0.0, 0.0, 0.8)), np.linalg.inv(drive["poses_cam"][1])]
    maps, refs = [m1, m2, m1], [r1, r2, r1]               # two entries name one map, with different frames
    want = [r.materialise(P) for r, P in zip(refs, invs)]
    x0 = np.asarray(drive["x_true"][3])

    def results(cs):
        out = []
        for cc, (cloud, off) in zip(cs, want):
            assert cc.cloud(True).tobytes() == cloud.tobytes() and np.array_equal(cc.ring_offsets(True), off)
            cc.set_source(*drive["frames"][4])
            out.append(register(cc, x0))
        return out

    for mm, cc, P in zip(maps, (a, b, c), invs):
        mm.load(cc, P)
    single = results((a, b, c))
    y.set_target(*want[2])
    y.set_source(*drive["frames"][4])
    assert register(y, x0) == single[2]
    api.map_load_batch(maps, [a, b, c], invs)
    assert results((a, b, c)) == single
    # alternate: single, batch in another order, single
    m2.load(a, invs[1])
    assert a.cloud(True).tobytes() == want[1][0].tobytes()
    api.map_load_batch([m1, m1, m2], [c, b, a], [invs[0], invs[2], invs[1]])
    assert c.cloud(True).tobytes() == want[0][0].tobytes() and b.cloud(True).tobytes() == want[2][0].tobytes() and a.cloud(True).tobytes() == want[1][0].tobytes()
    m1.load(b, invs[0])
    assert b.cloud(True).tobytes() == want[0][0].tobytes()
    api.map_load_batch([m2], [b], [invs[1]])              # n == 1 is the single entry
    assert b.cloud(True).tobytes() == want[1][0].tobytes()
    # an insert between loads on other streams, then a batch
    put(c, m2, r2, 2, *crafted([90, 91], 71), shift(0.0, 0.0, 1.6))
    api.map_load_batch([m2, m2], [a, b], [invs[1], EYE])
    assert a.cloud(True).tobytes() == r2.materialise(invs[1])[0].tobytes() and b.cloud(True).tobytes() == r2.materialise(EYE)[0].tobytes()
    # a batch with an empty map, a repeated context or a context list of another length changes nothing
    empty = api.ScanMap(0, 2, 100)
    keep = [cc.cloud(True).tobytes() for cc in (a, b)]
    with pytest.raises(api.VeloError, match="holds no scan"):
        api.map_load_batch([m2, empty], [a, b], [EYE, EYE])
    with pytest.raises(api.VeloError, match="same context"):
        api.map_load_batch([m2, m2], [a, a], [EYE, EYE])
    assert [cc.cloud(True).tobytes() for cc in (a, b)] == keep


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(ctxs, drive):
    c = ctxs[0]
    m, ref = api.ScanMap(0, 4, 1 << 20), R.ScanMapRef(4, 1 << 20)
    c.set_target(*drive["frames"][5])
    held = c.cloud(True).tobytes()
    with pytest.raises(api.VeloError, match="holds no scan"):       # an empty map
        m.load(c, EYE)
    assert c.cloud(True).tobytes() == held
    check_state(m, ref)
    put(c, m, ref, 0, *drive["frames"][0], EYE)
    put(c, m, ref, 1, *drive["frames"][1], drive["poses_cam"][1])
    c.set_source(*drive["frames"][2])
    with pytest.raises(api.VeloError, match="already"):             # a frame that is present
        m.insert(c, False, 1, EYE)
    for call in (lambda: m.drop(7), lambda: m.set_pose(7, EYE), lambda: m.get_scan(7)):      # an unknown frame
        with pytest.raises(api.VeloError, match="not in the map"):
            call()
    bad = EYE.copy()
    bad[0, 0] = np.inf
    with pytest.raises(api.VeloError, match="finite"):
        m.load(c, bad)
    with pytest.raises(api.VeloError, match="finite"):
        m.set_pose(1, bad)
    assert c.cloud(True).tobytes() == held
    check_state(m, ref)


# ---- what must not change --------------------------------------------------------------------------------------------------------------
def test_other_paths_are_unchanged_with_map_calls_in_between(ctxs, drive):
    a, y = ctxs[0], ctxs[1]
    m = api.ScanMap(0, 3, 1 << 20)
    cache_a, cache_y = api.ScanCache(0, 4), api.ScanCache(0, 4)
    x0 = np.asarray(drive["x_true"][0]) * 0.9
    out = {id(a): [], id(y): []}
    for c, cache, with_map in ((a, cache_a, True), (y, cache_y, False)):
        log = out[id(c)]
        c.set_target(*drive["frames"][0])
        c.set_source(*drive["frames"][1])
        if with_map:
            m.insert(c, True, 0, EYE)
            m.insert(c, False, 1, drive["poses_cam"][1])
        log.append(register(c, x0))                       # a frame-to-frame registration
        cache.store(1, c, False)
        cache.store(0, c, True)
        if with_map:
            m.load(c, EYE)                                # replaces the target ...
            m.insert(c, False, 2, EYE)
        cache.load(0, c, True)                            # ... which the cache brings back, index included
        cache.load(1, c, False)
        log.append(c.cloud(True).tobytes() + c.cloud(False).tobytes())
        log.append(register(c, x0))
        c.source_to_target()                              # the promotion
        if with_map:
            m.insert(c, True, 3, EYE)
        c.set_source(*drive["frames"][2])
        log.append(c.cloud(True).tobytes())
        log.append(register(c, np.asarray(drive["x_true"][1]) * 0.9))
    assert out[id(a)] == out[id(y)]
    assert m.frames() == [1, 2, 3]
