"""Holdout model evaluator (reference: autompc/evaluation/holdout_evaluator.py)."""
import numpy as np

from .evaluator import ModelEvaluator


class HoldoutModelEvaluator(ModelEvaluator):
    """Trains on the trajectories that are not held out and scores on the holdout set.

    The holdout is ``rng.choice(np.arange(n), round(holdout_prop * n), replace=False)``, sorted, exactly as the
    reference draws it (holdout_evaluator.py:37-43); the training set is every trajectory not EQUAL to a holdout
    one -- equality by value (Trajectory.__eq__), so a duplicate of a holdout trajectory is excluded too."""

    def __init__(self, *args, holdout_prop=0.1, holdout_set=None, verbose=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.verbose = verbose
        if holdout_set is None:
            holdout_size = round(holdout_prop * len(self.trajs))
            holdout_indices = self.rng.choice(np.arange(len(self.trajs)), holdout_size, replace=False)
            self.holdout_indices = sorted(int(i) for i in holdout_indices)
            self.holdout = [self.trajs[i] for i in self.holdout_indices]
        else:
            self.holdout_indices = None
            self.holdout = holdout_set
        self.training_set = []
        for traj in self.trajs:
            if traj not in self.holdout:
                self.training_set.append(traj)

    def __call__(self, model_factory, configuration):
        if self.verbose:
            print("Evaluating Configuration:")
            print(configuration)
            print("----")
        m = model_factory(configuration, self.training_set)
        return self.metric(m, self.holdout)

    def evaluate_batch(self, model_factory, configurations):
        """Scores of every configuration (one lockstep fit of the MLPs, one k-step kernel call per model
        shape; ``linear_kstep`` / ``sindy_kstep`` = "device" put the wide linear / SINDy models on the GPU too,
        ``mlp_kstep="batch"`` scores the MLPs of any mix of shapes in one launch);
        equal to ``[self(model_factory, cfg) for cfg in configurations]``."""
        return self._train_and_score(model_factory, list(configurations), self.training_set, self.holdout)
