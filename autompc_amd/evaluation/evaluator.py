"""Model evaluators: score a model configuration by prediction accuracy (reference:
autompc/evaluation/evaluator.py, holdout_evaluator.py).

``evaluator(factory, cfg)`` builds and trains one model and scores it, as the reference's does.
``evaluator.evaluate_batch(factory, cfgs)`` is the batched form the tuner uses: every model is built with
``skip_train_model=True``, the MLPs are fitted together by one ``sysid.mlp_fit.fit_mlps`` call (lockstep,
each model exactly as its own ``train()``), the others are trained one by one -- or, with ``linear_fit="device"``,
the ARX / Koopman models by one ``sysid.linear_fit.fit_linear_models`` call, with ``sindy_fit="device"`` the SINDy
models by one ``sysid.sindy_fit.fit_sindy_models`` call -- and all are scored by
``model_errors`` (one k-step kernel call per model shape; with ``linear_kstep="device"`` the ARX / Koopman models
wider than 64 states too, all of them in one ``ampc_kstep_errors_linear`` call, instead of the host loop; with
``sindy_kstep="device"`` the SINDy models in one ``ampc_kstep_errors_sindy`` call; with ``mlp_kstep="batch"`` the f64
MLPs of any mix of shapes in one ``ampc_kstep_errors_mlp`` call, read where the fit left them, no handle staged).

Deviation from the reference (bug not reproduced): the reference's ``"rmsmens"`` string raises ``NameError``
(evaluator.py:32-38: ``get_model_rmsmens`` is not imported and is called with ``horizon=``); here it scores
RMSMENS at the evaluator's horizon.
"""
from abc import ABC, abstractmethod

import numpy as np

from .model_metrics import METRICS, KstepReport, get_model_rmse, get_model_rmsmens, model_errors


class ModelEvaluator(ABC):
    """Evaluates models by prediction accuracy.  metric: "rmse", "rmsmens" or a callable
    ``(model, [Trajectory]) -> float``."""

    def __init__(self, system, trajs, metric, rng, horizon=1, linear_fit="host", linear_kstep="host",
                 sindy_kstep="host", sindy_fit="host", lasso_fit="host", stable_fit="host", mlp_fit="torch",
                 mlp_kstep="shape", sindy_wide_fit="host"):
        """linear_fit: how ``evaluate_batch`` fits ARX / Koopman models -- "host": each by its own ``train()``;
        "device": all of a batch by one ``sysid.linear_fit.fit_linear_models`` call (one Gram pass on the device,
        equal configurations fitted once).
        linear_kstep: how the string metrics score linear models wider than 64 states -- "host": the loop over
        ``pred_batch``; "device": one ``ampc_kstep_errors_linear`` call per batch (``model_errors``).
        sindy_kstep: how the string metrics score SINDy models -- "host": the loop over ``pred_batch``; "device":
        one ``ampc_kstep_errors_sindy`` call per batch.
        sindy_fit: how ``evaluate_batch`` fits SINDy models -- "host": each by its own ``train()``; "device": all of
        a batch by one ``sysid.sindy_fit.fit_sindy_models`` call (one Gram launch, equal configurations fitted once);
        ``last_sindy_fit`` holds its ``SindyFitReport``.
        sindy_wide_fit: with ``sindy_fit="device"``, how that call fits SINDy models whose library has 273..2048
        features -- "host": each by its own ``train()``; "device": by ``ampc_sindy_fit_wide``
        (``fit_sindy_models(..., wide="device")``).
        lasso_fit: with ``linear_fit="device"``, how that call fits Koopman models of method "lasso" -- "host": each
        by its own ``train()``; "device": by ``ampc_lasso_fit`` (``fit_linear_models(..., lasso="device")``).
        stable_fit: with ``linear_fit="device"``, how that call fits Koopman models of method "stable" -- "host": each
        by its own ``train()``, which refuses the method; "device": by ``ampc_stable_fit``, what it declines by
        ``sysid.stable_fit.stabilize_host`` (``fit_linear_models(..., stable="device")``).
        mlp_fit: how ``evaluate_batch`` fits MLP models -- "torch": the lockstep PyTorch fit (``fit_mlps``); "device":
        the library's own training kernels (``fit_mlps(..., fit="device")``, ampc_mlpfit_*: one launch chain for any
        mix of shapes); ``last_mlp_fit`` holds what the call returned.
        mlp_kstep: how the string metrics score MLP models -- "shape": one ``ampc_kstep_errors`` call per shape, one
        launch and one staged handle per model; "batch": one ``ampc_kstep_errors_mlp`` call for the f64 MLPs of any
        mix of depth, widths and activation, their parameters read in device memory where the fit left them
        (``model_errors(..., mlp_kstep="batch")``; ``last_kstep.mlp_batch_calls``).
        ``last_kstep`` holds the ``KstepReport`` of the last ``evaluate_batch`` (``host_fallbacks``)."""
        if linear_fit not in ("host", "device"):
            raise ValueError("linear_fit must be 'host' or 'device'")
        if linear_kstep not in ("host", "device"):
            raise ValueError("linear_kstep must be 'host' or 'device'")
        if sindy_kstep not in ("host", "device"):
            raise ValueError("sindy_kstep must be 'host' or 'device'")
        if sindy_fit not in ("host", "device"):
            raise ValueError("sindy_fit must be 'host' or 'device'")
        if sindy_wide_fit not in ("host", "device"):
            raise ValueError("sindy_wide_fit must be 'host' or 'device'")
        if lasso_fit not in ("host", "device"):
            raise ValueError("lasso_fit must be 'host' or 'device'")
        if stable_fit not in ("host", "device"):
            raise ValueError("stable_fit must be 'host' or 'device'")
        if mlp_fit not in ("torch", "device"):
            raise ValueError("mlp_fit must be 'torch' or 'device'")
        if mlp_kstep not in ("shape", "batch"):
            raise ValueError("mlp_kstep must be 'shape' or 'batch'")
        self.mlp_kstep = mlp_kstep
        self.mlp_fit = mlp_fit
        self.last_mlp_fit = None
        self.linear_fit = linear_fit
        self.lasso_fit = lasso_fit
        self.stable_fit = stable_fit
        self.sindy_fit = sindy_fit
        self.sindy_wide_fit = sindy_wide_fit
        self.last_sindy_fit = None
        self.linear_kstep = linear_kstep
        self.sindy_kstep = sindy_kstep
        self.last_kstep = None
        self.system = system
        self.trajs = trajs
        self.rng = rng
        self.horizon = int(horizon)
        if isinstance(metric, str):
            if metric == "rmse":
                self.metric = lambda model, trajs: get_model_rmse(model, trajs, horizon=self.horizon,
                                                                  linear_kstep=self.linear_kstep,
                                                                  sindy_kstep=self.sindy_kstep,
                                                                  mlp_kstep=self.mlp_kstep)
            elif metric == "rmsmens":
                self.metric = lambda model, trajs: get_model_rmsmens(model, trajs, horiz=self.horizon,
                                                                     linear_kstep=self.linear_kstep,
                                                                     sindy_kstep=self.sindy_kstep,
                                                                     mlp_kstep=self.mlp_kstep)
            else:
                raise ValueError("metric must be one of %s or a callable, not %r" % (", ".join(METRICS), metric))
            self.metric_name = metric
        elif callable(metric):
            self.metric, self.metric_name = metric, None
        else:
            raise ValueError("metric must be one of %s or a callable, not %r" % (", ".join(METRICS), metric))

    @abstractmethod
    def __call__(self, model_factory, configuration):
        """Score of the model `model_factory` builds from `configuration`."""
        raise NotImplementedError

    # -- the batched form ----------------------------------------------------------------------------
    def _train_and_score(self, model_factory, configurations, train_trajs, test_trajs):
        from ..sysid.mlp import MLP
        from ..sysid.mlp_fit import fit_mlps
        models = [model_factory(cfg, train_trajs, skip_train_model=True) for cfg in configurations]
        for m in models:
            # a model per configuration lives for one evaluation: no run-time kernel build for its shape
            m.jit_kernels = False
        mlps = [m for m in models if isinstance(m, MLP)]
        if mlps:
            self.last_mlp_fit = fit_mlps(mlps, train_trajs, fit=self.mlp_fit)
        others = [m for m in models if not isinstance(m, MLP)]
        if self.linear_fit == "device":
            from ..sysid.linear import ARX, Koopman
            from ..sysid.linear_fit import fit_linear_models
            linear = [m for m in others if isinstance(m, (ARX, Koopman))]
            if linear:
                self.last_linear_fit = fit_linear_models(linear, train_trajs, lasso=self.lasso_fit,
                                                             stable=self.stable_fit)
            others = [m for m in others if not isinstance(m, (ARX, Koopman))]
        if self.sindy_fit == "device":
            from ..sysid.sindy import SINDy
            from ..sysid.sindy_fit import fit_sindy_models
            sindys = [m for m in others if isinstance(m, SINDy)]
            if sindys:
                self.last_sindy_fit = fit_sindy_models(sindys, train_trajs, wide=self.sindy_wide_fit)
            others = [m for m in others if not isinstance(m, SINDy)]
        for m in others:
            m.train(train_trajs, silent=True)
        if self.metric_name is not None:
            self.last_kstep = KstepReport()
            return model_errors(models, test_trajs, [self.horizon], self.metric_name,
                                linear_kstep=self.linear_kstep, report=self.last_kstep,
                                sindy_kstep=self.sindy_kstep, mlp_kstep=self.mlp_kstep)[:, 0]
        return np.array([float(self.metric(m, test_trajs)) for m in models])
