"""Restatement of the device-resident scan map (velo_map_*) in plain Python / numpy: the window as a list of (frame, float32 cloud,
ring offsets, pose), the eviction rule, and materialise() with the sums written out left to right in float64 -- no `@`, no np.matmul,
so that no BLAS FMA can enter.  The GPU tests feed its cloud to velo_set_target on a second context: that is their yardstick."""
import numpy as np


def compose(a, b):
    """rows 0..2 of a @ b (row 3 copied from a @ b is not needed), every entry ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j"""
    a = np.asarray(a, dtype=np.float64).reshape(4, 4)
    b = np.asarray(b, dtype=np.float64).reshape(4, 4)
    m = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            m[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return m


def move(xyz, m):
    """q_i = ((M_i0 x + M_i1 y) + M_i2 z) + M_i3 in float64, rounded to float32 once"""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.stack([((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)], axis=1)
        return q.astype(np.float32)


def drop_empty_rings(off):
    off = np.asarray(off, dtype=np.int64)
    keep = np.concatenate([[True], off[1:] > off[:-1]])
    return off[keep].astype(np.int32)


class ScanMapRef:
    def __init__(self, max_scans, max_points):
        self.max_scans, self.max_points = int(max_scans), int(max_points)
        self.scans = []                                  # oldest first: [frame, xyz float32 [n, 3], offsets int32, pose [4, 4]]
        self.evictions = 0

    @property
    def points(self):
        return sum(len(s[1]) for s in self.scans)

    def find(self, frame):
        for k, s in enumerate(self.scans):
            if s[0] == frame:
                return k
        return -1

    def insert(self, frame, xyz, off, pose):
        """returns the number of evicted scans, or None when the scan is refused (the window is then as it was)"""
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        n = len(xyz)
        if n == 0 or n > self.max_points or self.find(frame) >= 0:
            return None
        gone = 0
        while self.scans and (len(self.scans) >= self.max_scans or self.points + n > self.max_points):
            self.scans.pop(0)
            gone += 1
        self.scans.append([int(frame), xyz.copy(), drop_empty_rings(off), np.asarray(pose, dtype=np.float64).reshape(4, 4).copy()])
        self.evictions += gone
        return gone

    def set_pose(self, frame, pose):
        self.scans[self.find(frame)][3] = np.asarray(pose, dtype=np.float64).reshape(4, 4).copy()

    def drop(self, frame):
        self.scans.pop(self.find(frame))

    def clear(self):
        self.scans = []

    def frames(self):
        return [s[0] for s in self.scans]

    def info(self):
        return dict(scans=len(self.scans), points=self.points, rings=sum(len(s[2]) - 1 for s in self.scans),
                    max_scans=self.max_scans, max_points=self.max_points, evictions=self.evictions)

    def materialise(self, ref_inv):
        """(cloud float32 [N, 3], ring offsets int32): scans oldest first, rings in scan order, all in the frame ref_inv names"""
        clouds, offs, at = [], [np.zeros(1, dtype=np.int64)], 0
        for _, xyz, off, pose in self.scans:
            clouds.append(move(xyz, compose(ref_inv, pose)))
            offs.append(off[1:].astype(np.int64) + at)
            at += len(xyz)
        return np.concatenate(clouds), np.concatenate(offs).astype(np.int32)
