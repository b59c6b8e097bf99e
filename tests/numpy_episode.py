"""Independent numpy restatement of one rr_episode_update (include/realrobot.h): what the device kernel does for every env, written
from the header's description and the reference's evaluateGoal (env.py:181-200), one env at a time in plain float32 numpy.

    score   sum over the goal's objects (flag bit 0) of exp(-(ln 4 / 0.10) |goal - position|), 0 without a goal
    reward  score - previous score (one float32 subtraction); the previous score becomes the score
    done    bit 0: timestep >= horizon > 0;  bit 1: errflags & 5
    reset   (reset_done and done != 0): index -> (index + stride) mod G, -1 stays -1; the objects with flag bit 1 take the new goal's
            start pose, the others their home pose; the previous score becomes the score of that start state; episode += 1
    goal_pos  the goal's positions where flag bit 0 is set, NaN elsewhere, all NaN without a goal

numpy's float32 exp / sqrt are not the device's: scores agree to a few ulp, everything else (bits, indices, masks, NaN pattern, the
subtraction) exactly.
"""
import numpy as np

POS_CONST = np.float32(-np.log(0.25) / 0.10)
SCORED, HAS_START = 1, 2


def score(obj_pos, final_pos, flags):
    """float32 score of one env: obj_pos [k, 3], final_pos [k, 3], flags [k]."""
    sc = np.float32(0.0)
    for i in range(len(flags)):
        if int(flags[i]) & SCORED:
            d = np.asarray(final_pos[i], np.float32) - np.asarray(obj_pos[i], np.float32)
            dist = np.sqrt(np.float32(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
            sc = np.float32(sc + np.exp(np.float32(-POS_CONST * dist)))
    return sc


def done_bits(timestep, errflags, horizon):
    t, e = np.asarray(timestep, np.int64), np.asarray(errflags, np.uint32)
    trunc = (t >= horizon) if horizon > 0 else np.zeros(t.shape, bool)
    return (trunc.astype(np.uint32) | (((e & 5) != 0).astype(np.uint32) << 1)).astype(np.uint32)


def next_index(index, stride, G):
    """(index + stride) mod G with Python's non-negative modulo; -1 (no goal) stays -1."""
    index = np.asarray(index, np.int64)
    out = index.copy()
    has = index >= 0
    if G > 0:
        out[has] = (index[has] + int(stride)) % G
    return out.astype(np.int32)


def goal_pos(index, final_pos, flags):
    """[N, k, 3]: the goal's position where the goal names the object, NaN elsewhere."""
    index = np.asarray(index)
    k = flags.shape[1] if np.ndim(flags) == 2 else 0
    out = np.full((len(index), k, 3), np.nan, np.float32)
    for e, gi in enumerate(index):
        if gi >= 0:
            named = (np.asarray(flags[gi]) & SCORED) != 0
            out[e, named] = np.asarray(final_pos[gi], np.float32)[named]
    return out


def start_positions(gi, home_pos, start_poses, flags):
    """[k, 3] positions an env starts its next episode from: the start pose where flag bit 1 is set, else the home position."""
    p = np.array(home_pos, np.float32)
    if gi >= 0:
        named = (np.asarray(flags[gi]) & HAS_START) != 0
        p[named] = np.asarray(start_poses[gi], np.float32)[named, :3]
    return p


class Record:
    """The per-env episode record and the table; `update` is one rr_episode_update."""

    def __init__(self, n_envs, start_poses, final_pos, flags, horizon=0, stride=1):
        self.start, self.final, self.flags = (np.asarray(start_poses, np.float32), np.asarray(final_pos, np.float32),
                                              np.asarray(flags, np.uint8))
        self.G = len(self.flags)
        self.horizon, self.stride = int(horizon), int(stride)
        self.index = np.full(n_envs, -1, np.int32)
        self.prev = np.zeros(n_envs, np.float32)
        self.episode = np.zeros(n_envs, np.int32)

    def _score(self, e, obj_pos):
        gi = self.index[e]
        return score(obj_pos, self.final[gi], self.flags[gi]) if gi >= 0 else np.float32(0.0)

    def set_env_goals(self, index, obj_pos, mask=None):
        """Stores the indices of the masked envs and re-bases their previous score to the score of obj_pos [N, k, 3]."""
        for e in range(len(self.index)):
            if mask is None or mask[e]:
                assert -1 <= index[e] < max(self.G, 0) or index[e] == -1
                self.index[e] = index[e]
                self.prev[e] = self._score(e, obj_pos[e])

    def update(self, obj_pos, timestep, errflags, reset_done, home_pos=None):
        """obj_pos [N, k, 3] and home_pos [N, k, 3] float32, timestep / errflags [N].  Returns dict(score, reward, done, reset
        (bool [N]: the envs that were reset), placed (bool [N, k]: the objects that took a start pose))."""
        n = len(self.index)
        sc = np.array([self._score(e, obj_pos[e]) for e in range(n)], np.float32)
        reward = (sc - self.prev).astype(np.float32)
        self.prev = sc.copy()
        done = done_bits(timestep, errflags, self.horizon)
        reset = (done != 0) & bool(reset_done)
        placed = np.zeros((n, obj_pos.shape[1]), bool)
        if reset.any():
            self.index = np.where(reset, next_index(self.index, self.stride, self.G), self.index).astype(np.int32)
            for e in np.flatnonzero(reset):
                gi = self.index[e]
                if gi >= 0:
                    placed[e] = (self.flags[gi] & HAS_START) != 0
                    self.prev[e] = score(start_positions(gi, home_pos[e], self.start, self.flags), self.final[gi], self.flags[gi])
                else:
                    self.prev[e] = np.float32(0.0)
                self.episode[e] += 1
        return {"score": sc, "reward": reward, "done": done, "reset": reset, "placed": placed}

    def goal_pos(self):
        return goal_pos(self.index, self.final, self.flags)
