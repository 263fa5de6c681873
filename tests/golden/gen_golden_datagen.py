#!/usr/bin/env python3
"""Golden trajectories of the data generators, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_datagen.py

Writes ``tests/golden/datagen_*.npz`` (data only).  Every case is one of the reference's
``autompc/utils/data_generation.py`` loops -- uniform_random_generate, random_walk_generate,
periodic_control_generate, multisine_generate (once with ``abort_if``) -- run on the reference's own ``System`` /
``Task`` with the project's test dynamics (tests/program_cases.py: pendulum2, a fresh array per call) and the
settings written there: a few trajectories of 8 steps from seeded ``numpy.random.default_rng`` generators.
Stored per case: ``lens`` [n], and ``obs`` [n][8][2] / ``ctrls`` [n][8][2] with each trajectory's rows first and
NaN after them (``abort_if`` shortens a trajectory).
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G                                        # noqa: E402  (installs the reference)
import program_cases as C                                     # noqa: E402
from autompc.utils import data_generation as ref              # noqa: E402


def main():
    system, task = C.pendulum_system_task(G.ampc.System, G.Task)
    with contextlib.redirect_stdout(io.StringIO()):           # (periodic_control_generate prints its periods)
        cases = C.generator_cases(ref, system, task, C.pendulum2)
    for name, trajs in cases.items():
        n = len(trajs)
        lens = np.array([len(t) for t in trajs], dtype=np.int64)
        obs = np.full((n, C.TRAJ_LEN, system.obs_dim), np.nan)
        ctrls = np.full((n, C.TRAJ_LEN, system.ctrl_dim), np.nan)
        for k, t in enumerate(trajs):
            obs[k, :lens[k]] = t.obs
            ctrls[k, :lens[k]] = t.ctrls
        path = os.path.join(HERE, "datagen_%s.npz" % name)
        np.savez(path, lens=lens, obs=obs, ctrls=ctrls)
        print("%s: %d trajectories, lengths %s -> %s" % (name, n, lens.tolist(), os.path.basename(path)))


if __name__ == "__main__":
    main()
