"""The five walks of the scene-set tests (CPU and GPU tiers): the shipped command, a slow, a lateral and a turning walk,
and one that starts with the left foot.  Built once per session and never modified."""
import functools

import numpy as np

from cmpc_amd import workloads as wl

#: name -> (velocity commands, first_swing, T, plan entries)
WALKS = {
    "shipped": (None, "rfoot", 1971, 20),
    "slow": ([(0.08, 0, 0)] * 10 + [(0, 0, 0)] * 3, "rfoot", 1271, 13),
    "lateral": ([(0.1, 0.03, 0)] * 8 + [(0, 0, 0)] * 3, "rfoot", 1071, 11),
    "turn": ([(0.1, 0, 0.15)] * 12 + [(0, 0, 0)] * 3, "rfoot", 1471, 15),
    "lfirst": ([(0.12, 0, 0)] * 9 + [(0, 0, 0)] * 3, "lfoot", 1171, 12),
}
NAMES = tuple(WALKS)


def walk_params(name, N=10):
    p = wl.default_params(N=N)
    p['first_swing'] = WALKS[name][1]
    return p


@functools.lru_cache(maxsize=None)
def five_scenes():
    return tuple(wl.Scene(walk_params(n), vref=WALKS[n][0]) for n in NAMES)


@functools.lru_cache(maxsize=None)
def scene_set():
    return wl.SceneSet(five_scenes())


def hw_for(name, hw):
    """The momentum recording for a walk: the left-first walk is the mirror image, so its signal is hw * (-1, 1, -1)."""
    return hw * np.array([-1.0, 1.0, -1.0]) if WALKS[name][1] == "lfoot" else hw
