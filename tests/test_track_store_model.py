"""The host model of the track store (track_store_model.py) against itself, without a GPU: a window built delta by delta, the way
tests/test_track_store.py hands it to the device, equals the same window flattened directly from the per-track observation sets."""
import numpy as np
import pytest

from track_store_model import TrackStoreModel, assert_frame_equal, assert_store_equal, bits_of, ragged_observations, same_bits


def window(seed, F, C, T):
    """per-feature observation sets as test_track_store.build draws them, measurements, points, and a track number per feature"""
    rng = np.random.default_rng(900 + seed)
    obs = ragged_observations(rng, F, C)
    uv = rng.normal(size=(F, C, 4))
    pf = rng.normal(size=(F, 3))
    track = np.random.default_rng(50 + seed).permutation(T)[:F]
    return obs, uv, pf, track


def flatten(obs, uv, pf, track, T, C):
    """the device layout straight from the observation sets: no deltas, no model"""
    mask = np.zeros(T, dtype=np.uint64); U = np.zeros((T, C, 4)); P = np.zeros((T, 3))
    for j, t in enumerate(track):
        for o in obs[j]:
            mask[t] |= np.uint64(1) << np.uint64(int(o))
            U[t, o] = uv[j, o]
        P[t] = pf[j]
    return mask, U, P


def column(obs, uv, track, s, slot, extra=()):
    js = [j for j in range(len(track)) if s in obs[j]]
    tr = [int(track[j]) for j in js] + [int(t) for t in extra]
    m = [uv[j, s] for j in js] + [np.full(4, 9.0)] * len(extra)
    return dict(append=slot, obs_track=tr, obs_uv=np.array(m).reshape(-1, 4))


@pytest.mark.parametrize("C,F,T", [(11, 40, 64), (36, 64, 513), (4, 24, 65536)])
def test_window_built_by_deltas_equals_the_flattened_window(C, F, T):
    obs, uv, pf, track = window(C, F, C, T)
    model = TrackStoreModel(T, C)
    junk = int(np.setdiff1d(np.arange(T), track)[0])
    reused = int(track[3])
    # two junk columns at slots 0 and 1, every track and a junk track observed ...
    for slot in (0, 1):
        model.apply(dict(append=slot, obs_track=[int(t) for t in track] + [junk], obs_uv=np.full((F + 1, 4), 7.0 + slot)))
    assert int(model.mask()[junk]) == 3
    # ... leave the window while the first real column arrives; the junk track is erased
    model.apply(dict(column(obs, uv, track, 0, 0), drop=[0, 1], free=[junk]))
    mid = C // 2
    for s in range(1, C - 1):
        if s == mid:                                                     # a column in the middle that leaves one delta later: the rows close up
            model.apply(dict(append=s, obs_track=[int(t) for t in track[:7]], obs_uv=np.full((7, 4), 3.0)))
            model.apply(dict(column(obs, uv, track, s, s), drop=[s]))
        elif s == mid + 1 and s < C - 1:
            # the track number is reused: its old observations are forgotten and the new owner's columns 0 .. s arrive one by one
            model.apply(dict(free=[reused]))
            assert model.obs[reused] == {}
            model.apply(column(obs, uv, track, s, s))
            j = 3
            for o in obs[j]:
                if o < s:
                    model.apply(dict(append=int(o), obs_track=[reused], obs_uv=uv[j, o].reshape(1, 4)))
        else:
            model.apply(column(obs, uv, track, s, s))
    model.apply(dict(column(obs, uv, track, C - 1, C - 1), pf_track=[int(t) for t in track], pf=pf))
    want = flatten(obs, uv, pf, track, T, C)
    assert_store_equal((model.mask(), model.uv(), model.pf()), want, C)
    assert same_bits(model.uv(), want[1])                               # the model keeps nothing stale
    # the gathered frame: features in an order unrelated to the tracks', with and without a selection
    order = np.random.default_rng(7).permutation(F)
    sel = np.random.default_rng(8).integers(0, 2 ** 63, size=F, dtype=np.uint64)
    for fs in (None, sel):
        g = model.gather(track[order], np.arange(F) % C, np.arange(F) % 256, fs, f_max=F + 5)
        mk = want[0][track[order]] if fs is None else want[0][track[order]] & fs
        assert np.array_equal(g["obs_mask"][:F], mk) and not g["obs_mask"][F:].any()
        assert same_bits(g["uv"], want[1][track[order]]) and same_bits(g["pf"], pf[order])
        assert np.array_equal(g["have"], bits_of(want[0][track[order]], C))
        assert_frame_equal(dict(g, obs_mask=g["obs_mask"].copy()), g, C, have=g["have"])


def test_drops_renumber_by_the_dropped_slots_below():
    m = TrackStoreModel(4, 8)
    for s in range(8):
        m.apply(dict(append=s, obs_track=[0, 1], obs_uv=np.full((2, 4), float(s))))
    m.apply(dict(drop=[0, 3, 7], append=5, obs_track=[1, 2], obs_uv=np.full((2, 4), 50.0), free=[1], pf_track=[1], pf=np.ones((1, 3))))
    assert sorted(m.obs[0]) == [0, 1, 2, 3, 4] and [m.obs[0][s][0] for s in range(5)] == [1.0, 2.0, 4.0, 5.0, 6.0]
    assert sorted(m.obs[1]) == [5] and sorted(m.obs[2]) == [5]            # freed and observed in one delta: only the new bit
    assert [int(x) for x in m.mask()] == [31, 32, 32, 0] and np.array_equal(m.pf()[1], np.ones(3))
