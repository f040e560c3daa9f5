"""Termination functions of the model-based rollouts (reference: utils/termination_fns.py).

Each ``termination_fn_*`` takes ``(obs, act, next_obs)`` as 2-D arrays and returns a ``[N, 1]`` done mask, with the reference's
outputs bit for bit, quirks included:
  * hopper's height-independent bound is ``abs(next_obs[:, 1:] < 100)``: the absolute value of a boolean, i.e. an upper bound only;
  * NaN / inf rows follow the numpy comparisons: halfcheetah, hopper, ant and walker2d mark them done (an ``isfinite`` or a range
    test fails), humanoid and pen compare false on NaN and leave them not done;
  * pendulum returns float zeros, door returns ``None``.

Functions that are a fixed row-wise test of ``next_obs`` carry a ``term_kind`` attribute (``TERM_*`` below), which names the test the
device rollout runs instead of the function (``orl_buffer_append_rollout``: ``EnsembleDynamics.term_kind`` ->
``policy.rollout_device`` -> ``DeviceBuffer.append_rollout``; the values are the C ABI's kind numbers).  ``obs_unnormalization``
wrappers, door and arbitrary callables carry none and are host only.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

# termination kinds (the row-wise tests above; 0 = never done)
TERM_NONE, TERM_HALFCHEETAH, TERM_HOPPER, TERM_WALKER2D, TERM_ANT, TERM_HUMANOID, TERM_PEN = range(7)


def _kind(k: int):
    def tag(fn):
        fn.term_kind = k
        return fn
    return tag


def _check(obs, act, next_obs) -> None:
    assert obs.ndim == 2 and act.ndim == 2 and next_obs.ndim == 2


def _never(obs) -> np.ndarray:
    return np.zeros((len(obs), 1), dtype=bool)


def term_kind(fn: Callable) -> Optional[int]:
    """the ``TERM_*`` kind of a termination function, or None for wrappers, door and arbitrary callables"""
    return getattr(fn, "term_kind", None)


def obs_unnormalization(termination_fn, obs_mean, obs_std):
    """wrap ``termination_fn`` so that it sees de-normalised observations (x * std + mean); host only"""
    def unnormalized(obs, act, next_obs):
        return termination_fn(obs * obs_std + obs_mean, act, next_obs * obs_std + obs_mean)
    return unnormalized


@_kind(TERM_HALFCHEETAH)
def termination_fn_halfcheetah(obs, act, next_obs):
    _check(obs, act, next_obs)
    inside = np.all(next_obs > -100, axis=-1) & np.all(next_obs < 100, axis=-1)
    return (~inside)[:, None]


@_kind(TERM_HOPPER)
def termination_fn_hopper(obs, act, next_obs):
    _check(obs, act, next_obs)
    z, ang = next_obs[:, 0], next_obs[:, 1]
    alive = (np.isfinite(next_obs).all(axis=-1) * np.abs(next_obs[:, 1:] < 100).all(axis=-1)
             * (z > .7) * (np.abs(ang) < .2))
    return (~alive)[:, None]


@_kind(TERM_NONE)
def termination_fn_halfcheetahveljump(obs, act, next_obs):
    _check(obs, act, next_obs)
    return _never(obs)


def _ant_like(obs, act, next_obs):
    _check(obs, act, next_obs)
    x = next_obs[:, 0]
    alive = np.isfinite(next_obs).all(axis=-1) * (x >= 0.2) * (x <= 1.0)
    return (~alive)[:, None]


@_kind(TERM_ANT)
def termination_fn_antangle(obs, act, next_obs):
    return _ant_like(obs, act, next_obs)


@_kind(TERM_ANT)
def termination_fn_ant(obs, act, next_obs):
    return _ant_like(obs, act, next_obs)


@_kind(TERM_WALKER2D)
def termination_fn_walker2d(obs, act, next_obs):
    _check(obs, act, next_obs)
    z, ang = next_obs[:, 0], next_obs[:, 1]
    alive = (np.logical_and(np.all(next_obs > -100, axis=-1), np.all(next_obs < 100, axis=-1))
             * (z > 0.8) * (z < 2.0) * (ang > -1.0) * (ang < 1.0))
    return (~alive)[:, None]


@_kind(TERM_NONE)
def termination_fn_point2denv(obs, act, next_obs):
    _check(obs, act, next_obs)
    return _never(obs)


@_kind(TERM_NONE)
def termination_fn_point2dwallenv(obs, act, next_obs):
    _check(obs, act, next_obs)
    return _never(obs)


@_kind(TERM_NONE)
def termination_fn_pendulum(obs, act, next_obs):
    _check(obs, act, next_obs)
    return np.zeros((len(obs), 1))


@_kind(TERM_HUMANOID)
def termination_fn_humanoid(obs, act, next_obs):
    _check(obs, act, next_obs)
    z = next_obs[:, 0]
    return ((z < 1.0) + (z > 2.0))[:, None]


@_kind(TERM_PEN)
def termination_fn_pen(obs, act, next_obs):
    _check(obs, act, next_obs)
    return (next_obs[:, 26] < 0.075)[:, None]       # z of the object position (columns 24:27)


def termination_fn_door(obs, act, next_obs):
    _check(obs, act, next_obs)
    return None                                     # the reference builds a mask and returns nothing


@_kind(TERM_NONE)
def termination_fn_default(obs, act, next_obs):
    _check(obs, act, next_obs)
    return _never(obs)


# substring tests in the reference's order: the first match wins, so the longer names come before their prefixes
_BY_NAME = (
    ("halfcheetahvel", termination_fn_halfcheetahveljump),
    ("halfcheetah", termination_fn_halfcheetah),
    ("hopper", termination_fn_hopper),
    ("antangle", termination_fn_antangle),
    ("ant", termination_fn_ant),
    ("walker2d", termination_fn_walker2d),
    ("point2denv", termination_fn_point2denv),
    ("point2dwallenv", termination_fn_point2dwallenv),
    ("pendulum", termination_fn_pendulum),
    ("humanoid", termination_fn_humanoid),
    ("pen", termination_fn_pen),
    ("door", termination_fn_door),
    ("maze", termination_fn_default),
)


def get_termination_fn(task):
    for key, fn in _BY_NAME:
        if key in task:
            return fn
    raise NotImplementedError
