"""Every growable host resource of the registration side across a context's life: the pinned slots and blocks, the events and streams
created on first use, the event pools of the timing levels, the exported slabs.  On ONE group of contexts every stage that owns such a
resource is called small and then large enough that the resource is freed and allocated again; ctxs[0] is the context that owns (or
leads the group that owns) all of them.  Every pose and summary of the grown group equals, byte for byte, what a fresh group gives for
that one call at that size; the same registrations at set_timing(3) give the same bytes and a non-empty kernel-time table; the group is
closed, a second life repeats everything, and the two lives are byte-identical.

What grows where (a pinned buffer of b bytes is allocated with b + b / 4 + 4096):
  pin[0..2]      set_target / set_source of a 16-beam pair, then of a 64-beam pair: 17 -> 65 ring offsets per table
  pin[3]         register_batch with a visual set of 8 matches, then 600 (68 bytes a match), on one context: the no-wait path of the
                 batch driver; a chained call's flags come back through the same slot
  h_batch        frame_to_frame_batch over 2 contexts, 3 and 6.  Six contexts run as three groups of two, so the block ctxs[0] leads is
                 sized for two again; the batch of three is one group of three, led by ctxs[0]
  pf.pin         hint_next_sources + register_batch with promote_refs on the 16-beam cloud, then on the 64-beam cloud; the call after
                 it takes the announced cloud out of the page-locked copy
  nf.call_done, src_bbox_ev
                 register_sequences over three frames, one drive (single-pair path) and two drives (one lock-step group)
  klog, assoc_events
                 all of the above at set_timing(3): every launch bracketed
  slabs, h_agree four comm_peer_export calls (two retired slabs are kept, the older ones freed), then a registration"""
import contextlib

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu

N_CTX = 6


@pytest.fixture(scope="module")
def cases():
    """inputs that do not depend on the device, made once for both lives"""
    pairs = [synth.scan_pair(n_beams=16, n_azimuth=400), synth.scan_pair(n_beams=64, n_azimuth=400)]
    for d in pairs:
        d["src_xyz"], d["tgt_xyz"] = np.ascontiguousarray(d["src_xyz"]), np.ascontiguousarray(d["tgt_xyz"])
    vis = [api.matches_from_dict(synth.stereo_matches(n // 2, seed=3 + n, mix="all", x_true=d["x_true"])) for n, d in zip((8, 600), pairs)]
    assert [len(v) for v in vis] == [8, 600]
    drives = [synth.drive(4, seed=40 + s, n_beams=16, n_azimuth=400) for s in range(2)]
    for d in drives:
        d["frames"] = [(np.ascontiguousarray(f[0]), f[1]) for f in d["frames"]]
    return dict(pairs=pairs, vis=vis, drives=drives)


def summary_bytes(s):
    """what a registration reports about its solves (the timing fields of the summary are not results)"""
    rows = [(v.termination, v.lm_iterations, v.evaluations, v.n_icp_valid, v.n_visual_blocks, v.initial_cost, v.final_cost)
            for v in (s.solves[k] for k in range(s.n_solves))]
    return np.asarray([(s.n_solves, s.n_assoc_rounds, s.n_queries, s.n_target, 0, 0, 0)] + rows, dtype=np.float64).tobytes()


def load(c, d):
    c.set_visual(None)                                                     # (an earlier step's matches are not part of this one)
    c.set_target(d["tgt_xyz"], d["tgt_off"])
    c.set_source(d["src_xyz"], d["src_off"])


def pair_step(k):
    def run(ctxs, cs):
        d = cs["pairs"][k]
        load(ctxs[0], d)
        x, T, s = ctxs[0].frame_to_frame(d["x0"])
        return [x.tobytes(), T.tobytes(), summary_bytes(s)]
    return run


def visual_step(k):
    def run(ctxs, cs):
        d, m = cs["pairs"][k], cs["vis"][k]
        x, T, S = api.register_batch(ctxs[:1], [(d["tgt_xyz"], d["tgt_off"])], [(d["src_xyz"], d["src_off"])], d["x0"][None, :], visual=api.visual_refs([m]))
        assert S[0].solves[0].n_visual_blocks > 0
        return [x.tobytes(), T.tobytes(), summary_bytes(S[0]), ctxs[0].good_matches().tobytes()]
    return run


def batch_step(n):
    def run(ctxs, cs):
        d = cs["pairs"][0]
        for c in ctxs[:n]:
            load(c, d)
        x, T, S = api.frame_to_frame_batch(ctxs[:n], [d["x0"]] * n)
        return [x.tobytes(), T.tobytes()] + [summary_bytes(s) for s in S]
    return run


def prefetch_step(k):
    def run(ctxs, cs):
        d = cs["pairs"][k]
        load(ctxs[0], d)
        nxt = api.scan_refs([(d["tgt_xyz"], d["tgt_off"])], 0)             # the frame announced: the old target comes back as the new source
        x0 = np.asarray(d["x0"])[None, :]
        api.hint_next_sources(ctxs[:1], nxt[0])
        out = []
        # the first call registers the loaded pair and copies the announced cloud into page-locked memory under its chain of launches; the
        # second promotes the source and reads the new one out of that copy
        for refs in (None, (api.promote_refs(1), nxt)):
            x, T, S = api.register_batch(ctxs[:1], None, None, x0, refs=refs)
            out += [x.tobytes(), T.tobytes(), summary_bytes(S[0])]
        return out
    return run


def sequence_step(n):
    def run(ctxs, cs):
        drives = cs["drives"][:n]
        for c, d in zip(ctxs, drives):
            c.set_visual(None)
            c.set_source(*d["frames"][0])
        refs, _keep, count = api.sequence_refs([d["frames"] for d in drives], 0, first=1)
        assert count == 3
        poses, guess = np.tile(np.eye(4), (n, 1, 1)), np.tile(synth.INITIAL_GUESS, (n, 1))
        xs, Ts, S = api.register_sequences(ctxs[:n], refs, count, poses, guess)
        return [xs.tobytes(), Ts.tobytes(), poses.tobytes(), guess.tobytes()] + [summary_bytes(s) for row in S for s in row]
    return run


STEPS = [("pair 16 beams", pair_step(0), 1), ("pair 64 beams", pair_step(1), 1), ("8 matches", visual_step(0), 1), ("600 matches", visual_step(1), 1),
         ("batch of 2", batch_step(2), 2), ("batch of 3", batch_step(3), 3), ("batch of 6", batch_step(6), 6),
         ("announced source, 16 beams", prefetch_step(0), 1), ("announced source, 64 beams", prefetch_step(1), 1),
         ("one drive of three frames", sequence_step(1), 1), ("two drives of three frames", sequence_step(2), 2)]


@contextlib.contextmanager
def group(n):
    ctxs = [api.Context(0, icp_skip=1) for _ in range(n)]
    try:
        yield ctxs
    finally:
        for c in ctxs:
            c.close()


@pytest.fixture(scope="module")
def fresh(cases):
    """every step on a group of its own that has done nothing else, computed once"""
    out = {}
    for name, step, n in STEPS:
        with group(n) as ctxs:
            out[name] = step(ctxs, cases)
    return out


def one_life(cases, fresh):
    out, differ = [], []
    with group(N_CTX) as ctxs:
        for name, step, _ in STEPS:
            got = step(ctxs, cases)
            if got != fresh[name]:
                differ.append(name)
            out += got
        for c in ctxs:
            c.set_timing(3)
        ctxs[0].kernel_times(reset=True)
        for name, step, _ in STEPS:                                        # every launch bracketed: the event pools grow call by call
            if step(ctxs, cases) != fresh[name]:
                differ.append(f"{name}, timed")
        assert not differ, f"not what a fresh group gives: {differ}"
        times = ctxs[0].kernel_times()
        assert times and all(launches > 0 for _, launches, _ in times.values())
        for c in ctxs:
            c.set_timing(0)
        for _ in range(4):                                                 # every export hands out a new slab; the retired ones are capped at two
            assert len(ctxs[0].comm_peer_export()) == 64
        got = pair_step(0)(ctxs, cases)
        assert got == fresh["pair 16 beams"], "after the exports"
        out += got
    return out


def test_grown_context_equals_fresh_ones_and_its_second_life(cases, fresh):
    first = one_life(cases, fresh)
    second = one_life(cases, fresh)
    assert len(first) == len(second) > 40
    assert all(a == b for a, b in zip(first, second))
