"""Batch ask/tell model tuner: searches model configurations by prediction accuracy.

What it replaces.  ``ModelTuner.run`` (reference autompc/tuning/model_tuner.py:115-199) hands SMAC one
``evaluator(factory, cfg)`` at a time over a combined configuration space -- a categorical ``"model"`` (the
factory name) and every factory's space under the prefix ``"_<name>:"`` (:141-150) -- and afterwards walks
SMAC's run history into a ``ModelTuneResult`` (:168-190); the returned model is the incumbent configuration
trained on ALL of ``evaluator.trajs`` (:196-197).  ``PipelineTuner``'s ``surrogate_mode="autotune"`` /
``"autoselect"`` (pipeline_tuner.py:116-150) run it to pick the surrogate.

Here configurations are proposed in batches (``ask``), a whole batch is scored at once -- the evaluator's
``evaluate_batch`` fits every MLP of the batch in one lockstep fit and scores all models with one k-step
kernel call per shape (evaluation/), sharded over the ranks of the default ``torch.distributed`` group by
``evaluate_sharded`` -- and reported back (``tell``).  The proposal rule is random search over the factories'
ranges (the default sampler covers ``MLPFactory``, ``ARXFactory`` and ``KoopmanFactory`` through
``sample_mlp_config`` / ``sample_arx_config`` / ``sample_koopman_config``); any other proposer drives
``ask`` / ``tell`` through ``sampler=`` or passes ``configs=`` to ``run``.  Scores that are not finite count as
``inf``; only a strict improvement replaces the incumbent.
"""
from collections import namedtuple

import numpy as np

from .batch_eval import evaluate_sharded
from .configs import DictConfiguration, config_dict, sample_arx_config, sample_koopman_config, sample_mlp_config

# same fields, same order as the reference's namedtuple (model_tuner.py:37-38)
ModelTuneResult = namedtuple("ModelTuneResult", ["inc_cfg", "cfgs", "inc_cfgs", "costs", "inc_costs"])


class BatchModelTuner:
    """evaluator: a ``ModelEvaluator`` (``evaluate_batch(factory, cfgs) -> scores`` is used when it has one,
    else ``evaluator(factory, cfg)`` per configuration) with the full data set as ``evaluator.trajs``.  The
    evaluator's own options decide where a batch's linear models are fitted and scored (``linear_fit="device"``,
    ``linear_kstep="device"``: ARX / Koopman models wider than 64 states in one k-step launch;
    ``sindy_kstep="device"``: a batch's SINDy models in one k-step launch; ``sindy_fit="device"``: their thresholded
    fits in one ``ampc_sindy_fit`` call, with ``sindy_wide_fit="device"`` those of 273..2048 features in one
    ``ampc_sindy_fit_wide`` call; ``mlp_fit="device"``: a batch's MLPs by the library's training kernels;
    ``mlp_kstep="batch"``: a batch's MLPs of any mix of shapes scored by one ``ampc_kstep_errors_mlp`` launch, read where
    the fit left them).
    sampler: ``sampler(tuner, n, rng) -> n combined configurations``; the default draws a factory uniformly and
    its configuration from its ranges (``MLPFactory`` / ``ARXFactory`` / ``KoopmanFactory``: ``sample_mlp_config`` /
    ``sample_arx_config`` / ``sample_koopman_config``; other factories need a
    ``sample_configuration(rng)`` method, ``sampler=`` or ``run(..., configs=...)``)."""

    def __init__(self, system, evaluator, batch_size=64, sampler=None, sindy_wide_fit=None):
        """sindy_wide_fit: None leaves the evaluator as it is; "host" / "device" sets the evaluator's option of that
        name (``ModelEvaluator``: with ``sindy_fit="device"``, SINDy libraries of 273..2048 features fitted by
        ``ampc_sindy_fit_wide``)."""
        self.system, self.evaluator = system, evaluator
        if sindy_wide_fit is not None:
            if sindy_wide_fit not in ("host", "device"):
                raise ValueError("sindy_wide_fit must be 'host' or 'device'")
            evaluator.sindy_wide_fit = sindy_wide_fit
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self._sampler = sampler
        self.model_factories = []
        self.reset()

    def reset(self):
        self.cfgs, self.costs, self.inc_cfgs, self.inc_costs = [], [], [], []
        self._inc_cfg, self._inc_cost = None, float("inf")

    def add_model_factory(self, model_factory):
        """A factory the search may choose (model_tuner.py:82-100); its ``name`` prefixes its keys."""
        self.model_factories.append(model_factory)

    # -- combined configurations (model_tuner.py:102-113, :141-150) ------------------------------------
    @staticmethod
    def _prefix(factory):
        return "_" + factory.name + ":"

    def combined_config(self, factory, cfg):
        """The combined configuration: ``"model"`` = factory name, ``"_<name>:<key>"`` = value."""
        out = DictConfiguration(model=factory.name)
        for k, v in config_dict(cfg).items():
            out[self._prefix(factory) + k] = v
        return out

    def model_config(self, cfg_combined):
        """(factory, its sub-configuration) of a combined configuration (model_tuner.py:102-110)."""
        d = config_dict(cfg_combined)
        name = d.get("model")
        if name is None and len(self.model_factories) == 1:
            name = self.model_factories[0].name
        for factory in self.model_factories:
            if factory.name != name:
                continue
            pre = self._prefix(factory)
            return factory, DictConfiguration({k.split(":", 1)[1]: v for k, v in d.items() if k[:len(pre)] == pre})
        raise ValueError("configuration names model %r, which no added factory provides" % (name,))

    def _random_search(self, n, rng):
        if not self.model_factories:
            raise ValueError("no model factory added (add_model_factory)")
        out = []
        for _ in range(n):
            k = int(rng.integers(len(self.model_factories))) if len(self.model_factories) > 1 else 0
            factory = self.model_factories[k]
            from ..sysid.linear import ARXFactory, KoopmanFactory
            from ..sysid.mlp import MLPFactory
            if isinstance(factory, MLPFactory):
                cfg = sample_mlp_config(rng)
            elif hasattr(factory, "sample_configuration"):
                cfg = factory.sample_configuration(rng)
            elif isinstance(factory, ARXFactory):
                cfg = sample_arx_config(rng)
            elif isinstance(factory, KoopmanFactory):
                cfg = sample_koopman_config(rng)
            else:
                raise ValueError("the default sampler covers MLPFactory, ARXFactory and KoopmanFactory: pass sampler= or "
                                 "run(..., configs=...) for %s" % factory.name)
            out.append(self.combined_config(factory, cfg))
        return out

    # -- ask / tell ------------------------------------------------------------------------------------
    def ask(self, n, rng):
        """The next `n` combined configurations to evaluate."""
        cfgs = list(self._sampler(self, int(n), rng) if self._sampler is not None else self._random_search(int(n), rng))
        if len(cfgs) != n:
            raise ValueError("sampler returned %d configurations, %d asked" % (len(cfgs), n))
        return cfgs

    def tell(self, cfgs, scores):
        """Record evaluated configurations in order: the incumbent trace of model_tuner.py:177-185 (strict
        improvement replaces; a non-finite score counts as inf)."""
        scores = np.asarray(scores, dtype=np.float64)
        if len(cfgs) != scores.shape[0]:
            raise ValueError("one score per configuration expected")
        for cfg, s in zip(cfgs, scores):
            s = float(s) if np.isfinite(s) else float("inf")
            if s < self._inc_cost or self._inc_cfg is None:
                self._inc_cost, self._inc_cfg = s, cfg
            self.cfgs.append(cfg)
            self.costs.append(s)
            self.inc_cfgs.append(self._inc_cfg)
            self.inc_costs.append(self._inc_cost)

    def result(self):
        return ModelTuneResult(inc_cfg=self._inc_cfg, cfgs=list(self.cfgs), inc_cfgs=list(self.inc_cfgs),
                               costs=list(self.costs), inc_costs=list(self.inc_costs))

    # -- the loop --------------------------------------------------------------------------------------
    def evaluate(self, cfgs):
        """Scores of combined configurations in order: per factory one ``evaluate_batch`` call (or one
        evaluator call per configuration)."""
        scores = np.empty(len(cfgs))
        by_factory = {}
        for i, c in enumerate(cfgs):
            factory, sub = self.model_config(c)
            by_factory.setdefault(id(factory), (factory, [], []))
            by_factory[id(factory)][1].append(i)
            by_factory[id(factory)][2].append(sub)
        for factory, idx, subs in by_factory.values():
            if hasattr(self.evaluator, "evaluate_batch"):
                scores[idx] = np.asarray(self.evaluator.evaluate_batch(factory, subs), dtype=np.float64)
            else:
                scores[idx] = [float(self.evaluator(factory, s)) for s in subs]
        return scores

    def run(self, rng, n_iters=10, configs=None):
        """Evaluate `n_iters` configurations in batches of `batch_size` -- sampled, or the first `n_iters` of
        `configs` (combined configurations) in order -- and return (model, ModelTuneResult): the model is the
        incumbent configuration trained on all of ``evaluator.trajs`` (model_tuner.py:196-197).  Every rank
        must call this with an identically seeded `rng`; each scores its shard of every batch."""
        if configs is not None and len(configs) < n_iters:
            raise ValueError("%d configurations given, %d evaluations asked" % (len(configs), n_iters))
        done = 0
        while done < n_iters:
            n = min(self.batch_size, n_iters - done)
            batch = list(configs[done:done + n]) if configs is not None else self.ask(n, rng)
            scores = evaluate_sharded(lambda shard, lo: self.evaluate(shard), batch)
            self.tell(batch, scores)
            done += n
        if self._inc_cfg is None:
            return None, self.result()
        factory, sub = self.model_config(self._inc_cfg)
        return factory(sub, self.evaluator.trajs), self.result()
