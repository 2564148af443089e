"""The landmark bookkeeping of the reference's frame loop, transcribed literally into Python containers (dicts of dicts where the
reference has vectors of std::map, sorted(set) where it has std::set): main.cpp:614-645 (accumulate keypoint_obs2 / keypoint_obs3 /
keypoint_obs_count), main.cpp:647-679 (which ids are triangulated, keypoint_added), velo.h:1049-1122 (the order in which
triangulatePoint adds a landmark's residual blocks) and velo.h:1132-1160 (getLandmarksAtFrame).  It solves nothing: csr() emits the
arguments of the stateless velo_triangulate_points, store() takes its results back.  Also here: the seeded synthetic sequences the
landmark tests walk."""
import numpy as np

from velo_amd import synth

TRI_OBS_DTYPE = np.dtype([("kind", np.int32), ("frame", np.int32), ("cam", np.int32), ("s", np.float32, 3)])


class LandmarkBook:
    def __init__(self, num_cams: int):
        self.num_cams = num_cams
        self.keypoint_obs2 = []        # [id][cam] -> {frame: (x, y)}
        self.keypoint_obs3 = []        # [id][cam] -> {frame: (x, y, z)}
        self.keypoint_obs_count = []
        self.keypoint_added = []
        self.landmarks = []            # [id] -> float32[3]
        self.keypoint_ids = {}         # [cam][frame] -> ids

    def observe_frame(self, frame, keypoints, keypoint_ids, has_depth, kp_with_depth):
        """main.cpp:614-645; the arguments are this frame's keypoints[cam], keypoint_ids[cam], has_depth[cam], kp_with_depth[cam]"""
        id_counter = max([len(self.keypoint_added) - 1] + [int(i) for cam in range(self.num_cams) for i in keypoint_ids[cam]])
        while len(self.keypoint_added) < id_counter + 1:              # the resize calls of main.cpp:614-621
            self.keypoint_added.append(False)
            self.landmarks.append(np.zeros(3, dtype=np.float32))
            self.keypoint_obs_count.append(0)
            self.keypoint_obs2.append([dict() for _ in range(self.num_cams)])
            self.keypoint_obs3.append([dict() for _ in range(self.num_cams)])
        for cam in range(self.num_cams):
            self.keypoint_ids.setdefault(cam, {})[frame] = [int(i) for i in keypoint_ids[cam]]
            for i in range(len(keypoints[cam])):
                id = int(keypoint_ids[cam][i])
                self.keypoint_obs_count[id] += 1
                if has_depth[cam][i] == -1:
                    self.keypoint_obs2[id][cam][frame] = np.asarray(keypoints[cam][i], dtype=np.float32)
                else:
                    self.keypoint_obs3[id][cam][frame] = np.asarray(kp_with_depth[cam][has_depth[cam][i]], dtype=np.float32)

    def ids_to_triangulate(self, frame):
        """main.cpp:647-657"""
        ids_seen = set()
        for cam in range(self.num_cams):
            for id in self.keypoint_ids.get(cam, {}).get(frame, []):
                ids_seen.add(id)
        return [id for id in sorted(ids_seen) if self.keypoint_obs_count[id] >= 3]

    def csr(self, ids):
        """velo.h:1043-1122 for every id: (obs, obs_offsets, points0, initial_guess)"""
        rows, off = [], [0]
        for id in ids:
            for cam in range(self.num_cams):
                for frame in sorted(self.keypoint_obs3[id][cam]):            # std::map iterates in key order
                    rows.append((0, frame, cam, self.keypoint_obs3[id][cam][frame]))
            for cam in range(self.num_cams):
                for frame in sorted(self.keypoint_obs2[id][cam]):
                    p = self.keypoint_obs2[id][cam][frame]
                    rows.append((1, frame, cam, np.array([p[0], p[1], 0.0], dtype=np.float32)))
            off.append(len(rows))
        obs = np.zeros(len(rows), dtype=TRI_OBS_DTYPE)
        for k, (kind, frame, cam, s) in enumerate(rows):
            obs[k] = (kind, frame, cam, s)
        points0 = np.array([self.landmarks[id] for id in ids], dtype=np.float32).reshape(-1, 3)
        init = np.array([self.keypoint_added[id] for id in ids], dtype=np.uint8)
        return obs, np.asarray(off, dtype=np.int32), points0, init

    def store(self, ids, points):
        """main.cpp:661-678: landmarks->at(id) = the solved point, keypoint_added[id] = true"""
        for id, p in zip(ids, points):
            self.landmarks[id] = np.asarray(p, dtype=np.float32).copy()
            self.keypoint_added[id] = True

    def landmarks_at_frame(self, poseinv, frame):
        """velo.h:1132-1160 with the inverse handed in; the product row by row, summed left to right in double.  Returns the
        std::map as (ids ascending, xyz float32)."""
        M = np.asarray(poseinv, dtype=np.float64).reshape(4, 4)
        out = {}
        for cam in range(self.num_cams):
            for id in self.keypoint_ids.get(cam, {}).get(frame, []):
                if id in out:
                    continue
                if not self.keypoint_added[id]:
                    continue
                q = [np.float64(self.landmarks[id][0]), np.float64(self.landmarks[id][1]), np.float64(self.landmarks[id][2]), np.float64(1.0)]
                p = [((M[r, 0] * q[0] + M[r, 1] * q[1]) + M[r, 2] * q[2]) + M[r, 3] * q[3] for r in range(4)]
                out[id] = np.array([p[0] / p[3], p[1] / p[3], p[2] / p[3]]).astype(np.float32)
        ids = sorted(out)
        return np.asarray(ids, dtype=np.int32), np.array([out[i] for i in ids], dtype=np.float32).reshape(-1, 3)


def sequence(seed: int, n_frames: int, n_cams: int, ids, first_frame=None, long_ids=(), empty_frames=(), sigma_2d=7e-4, sigma_3d=0.03):
    """A seeded drive: poses [F, 6], cam_trans [n_cams, 3] and per frame, per camera (ids, keypoints [n, 2], has_depth [n],
    kp_with_depth [m, 3]) in shuffled order.  `ids` live in a window of frames from first_frame[id] (default: a random one) and are
    seen by each camera with probability 0.8 (so they skip frames and cameras); id % 7 == 0 always has LiDAR depth (3-D only),
    id % 7 == 1 never (2-D only), the others sometimes.  long_ids: (id, cams) seen in EVERY non-empty frame by those cameras.
    empty_frames: nobody sees anything."""
    rng = np.random.default_rng(seed)
    F = n_frames
    k = np.arange(F, dtype=np.float64)
    poses = np.stack([0.002 * np.sin(0.7 * k), 0.004 * k, 0.001 * np.cos(0.5 * k), 0.02 * k, 0.01 * np.sin(k), 0.3 * k], axis=1)
    poses[0] = 0.0
    R = [synth.rotvec_to_matrix(p[:3]) for p in poses]
    tc = synth.CAM_TRANS[:n_cams].astype(np.float64)
    truth, window = {}, {}
    for id in ids:
        f0 = int(rng.integers(0, F)) if first_frame is None or id not in first_frame else first_frame[id][0]
        ln = int(rng.integers(1, 9)) if first_frame is None or id not in first_frame else first_frame[id][1]
        z = 6.0 + 40.0 * rng.random()
        truth[id] = np.array([(rng.random() - 0.5) * 1.2 * z, (rng.random() - 0.5) * 0.4 * z, z]) + poses[min(f0, F - 1), 3:]
        window[id] = (f0, f0 + ln)
    for id, _ in long_ids:
        truth[id] = np.array([3.0 * rng.random(), 1.0 * rng.random(), 90.0 + 10 * rng.random()])
    frames = []
    for f in range(F):
        per_cam = []
        for cam in range(n_cams):
            rows = []
            if f not in empty_frames:
                seen = [id for id in ids if window[id][0] <= f < window[id][1] and rng.random() < 0.8]
                seen += [id for id, cams in long_ids if cam in cams]
                for id in seen:
                    M = R[f].T @ (truth[id] - poses[f, 3:])
                    if M[2] < 1.0:
                        continue
                    Mc = M + tc[cam]
                    kp = Mc[:2] / Mc[2] + sigma_2d * rng.normal(size=2)
                    depth = id % 7 == 0 or (id % 7 != 1 and rng.random() < 0.4)
                    rows.append((id, kp, (M + sigma_3d * rng.normal(size=3)) if depth else None))
            order = rng.permutation(len(rows))
            rows = [rows[i] for i in order]
            with_depth = [i for i, r in enumerate(rows) if r[2] is not None]
            slot = {i: s for s, i in enumerate(rng.permutation(with_depth))} if with_depth else {}
            cloud = np.zeros((len(with_depth), 3), dtype=np.float32)
            for i, s in slot.items():
                cloud[s] = rows[i][2]
            per_cam.append((np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.float32).reshape(-1, 2),
                            np.array([slot.get(i, -1) for i in range(len(rows))], dtype=np.int32), cloud))
        frames.append(per_cam)
    return dict(poses=poses, cam_trans=synth.CAM_TRANS[:n_cams].astype(np.float32).copy(), frames=frames, n_cams=n_cams)


def main_sequence():
    """66 frames, 2 cameras, about 200 ids in the last 12 frames.  Id 5 is seen by both cameras and id 70000 by camera 0 in every
    frame but the empty one (60): id 5 passes 64 observations and ends at 130, id 70000 passes 64 and ends at 65.  Ids 50..53 end
    with 0, 1, 2 (both cameras of one frame) and 3 observations."""
    ids = list(range(100, 300))
    first = {51: (56, 1), 52: (57, 1), 53: (58, 2)}
    seq = sequence(2024, 66, 2, ids, long_ids=((5, (0, 1)), (70000, (0,))), empty_frames=(60,),
                   first_frame={id: (54 + (id * 7) % 12, 1 + (id * 5) % 9) for id in ids})
    # the hand-placed short lives, appended to what the generator made (2-D entries at plausible coordinates)
    def put(frame, cam, id, xy):
        i, k, h, c = seq["frames"][frame][cam]
        seq["frames"][frame][cam] = (np.append(i, np.int32(id)), np.vstack([k, np.asarray(xy, np.float32)[None]]).astype(np.float32),
                                     np.append(h, np.int32(-1)), c)
    put(first[51][0], 0, 51, (0.01, 0.02))
    put(first[52][0], 0, 52, (0.03, -0.02)); put(first[52][0], 1, 52, (0.05, -0.02))
    put(58, 0, 53, (-0.04, 0.01)); put(58, 1, 53, (-0.02, 0.01)); put(59, 0, 53, (-0.041, 0.011))
    return seq
