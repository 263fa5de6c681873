"""The reference's pipeline ``Configuration`` <-> the evaluators' candidate dictionaries.

What it replaces.  The reference searches ONE joint ConfigSpace built by ``Pipeline.get_configuration_space``
(autompc/pipeline.py:90-105): the model factory's space under the prefix ``_model:``, the controller factory's
under ``_ctrlr:``, the cost factory's under ``_cost:``.  ``Pipeline.__call__`` (pipeline.py:107-168) splits a
configuration back into the three sub-configurations (``set_subspace_configuration``, utils/cs_utils.py:33-37:
every key that starts with the prefix, prefix stripped) and hands each to its factory:

    _ctrlr:horizon | sigma | lmda | num_path         MPPIFactory (control/mppi.py:48-64); iLQR: horizon only
                                                     (control/ilqr.py:36-41)
    _cost:<obs>_Q | <obs>_F | <ctrl>_R               QuadCostFactory (costs/quad_cost_factory.py:40-95): diagonal
                                                     gains by observation / control NAME; an absent key is gain 0
    _model:nonlintype | n_hidden_layers | hidden_size_1..4 | lr    MLPFactory (sysid/mlp.py:107-135)

``candidate_from_config`` performs that split for the batched evaluators (``CandidateEvaluator`` /
``IlqrCandidateEvaluator`` take dicts with horizon, sigma, lmda, num_path, Q, R, F and optionally ``model`` /
``model_cfg``); ``config_from_candidate`` is the inverse, so that what a tuner reports as ``inc_cfg`` is
something ``Pipeline.__call__`` accepts.  LQRFactory's sub-space (``_ctrlr:finite_horizon`` and, when it is
"true", ``_ctrlr:horizon``; control/lqr.py:214-224) has its own entry point, ``lqr_candidate_from_config``, for
``LqrCandidateEvaluator``; ``candidate_from_config`` refuses it, so an LQR configuration is never scored as an iLQR
one of the same horizon.  ``sample_arx_config`` / ``sample_koopman_config`` draw the linear models' sub-spaces and
``sample_lqr_pipeline_configs`` whole LQR pipeline configurations.  Configurations are read through ``get_dictionary()`` (ConfigSpace's
``Configuration``) or as plain mappings; ``DictConfiguration`` is the minimal object with that method, used
where ConfigSpace itself is not installed.  ``sample_pipeline_configs`` draws from the factories' ranges with
the reference's key names (what ``cs.sample_configuration(n)`` / SMAC's initial design would produce).
"""
import numpy as np

MODEL, CTRLR, COST = "_model", "_ctrlr", "_cost"
_MPPI_KEYS = ("sigma", "lmda", "num_path")


class DictConfiguration(dict):
    """A mapping that answers ``get_dictionary()`` like ConfigSpace's ``Configuration``."""

    def get_dictionary(self):
        return dict(self)


def config_dict(cfg):
    """The plain {name: value} view of a ConfigSpace ``Configuration`` or of a mapping."""
    if hasattr(cfg, "get_dictionary"):
        return dict(cfg.get_dictionary())
    return dict(cfg)


def subspace(d, prefix, delimiter=":"):
    """Entries of `d` under `prefix`, prefix stripped (cs_utils.set_subspace_configuration)."""
    pre = prefix + delimiter
    return {k[len(pre):]: v for k, v in d.items() if k[:len(pre)] == pre}


def candidate_from_config(system, cfg):
    """One evaluator candidate from a pipeline configuration; the configuration itself rides along under
    ``"cfg"`` (tuners report it back unchanged)."""
    d = config_dict(cfg)
    ctrl, cost, model = subspace(d, CTRLR), subspace(d, COST), subspace(d, MODEL)
    if "finite_horizon" in ctrl:
        # LQRFactory's sub-space (control/lqr.py:214-224): refused here, before the fall-through below would score
        # it as an iLQR candidate of the same horizon; lqr_candidate_from_config maps it for LqrCandidateEvaluator
        raise NotImplementedError("%s:finite_horizon: an LQR configuration is not an MPPI / iLQR candidate; map it "
                                  "with lqr_candidate_from_config and score it with LqrCandidateEvaluator" % CTRLR)
    if "horizon" not in ctrl:
        raise KeyError("configuration has no %s:horizon (MPPIFactory / IterativeLQRFactory sub-space)" % CTRLR)
    cand = {"horizon": int(ctrl["horizon"])}
    if any(k in ctrl for k in _MPPI_KEYS):
        missing = [k for k in _MPPI_KEYS if k not in ctrl]
        if missing:
            raise KeyError("MPPI configuration lacks %s" % ", ".join("%s:%s" % (CTRLR, k) for k in missing))
        cand.update(sigma=float(ctrl["sigma"]), lmda=float(ctrl["lmda"]), num_path=int(ctrl["num_path"]))
    _cost_and_model(system, cand, cost, model)
    cand["cfg"] = cfg
    return cand


def _cost_and_model(system, cand, cost, model):
    # QuadCostFactory.__call__ (quad_cost_factory.py:73-92): gains by name, absent -> 0
    cand["Q"] = np.array([float(cost.get("%s_Q" % n, 0.0)) for n in system.observations])
    cand["F"] = np.array([float(cost.get("%s_F" % n, 0.0)) for n in system.observations])
    cand["R"] = np.array([float(cost.get("%s_R" % n, 0.0)) for n in system.controls])
    if model:
        cand["model_cfg"] = dict(model)


def lqr_candidate_from_config(system, cfg):
    """One LqrCandidateEvaluator candidate from an (ARX | Koopman) x LQR x QuadCost pipeline configuration:
    ``_ctrlr:finite_horizon`` ("true" / "false" or a bool), ``_ctrlr:horizon`` (required only when finite), the
    ``_cost:`` gains as candidate_from_config reads them and the ``_model:`` sub-space as ``model_cfg``.  The
    configuration rides along under ``"cfg"``."""
    from .lqr_eval import is_finite_horizon
    d = config_dict(cfg)
    ctrl, cost, model = subspace(d, CTRLR), subspace(d, COST), subspace(d, MODEL)
    if "finite_horizon" not in ctrl:
        raise KeyError("configuration has no %s:finite_horizon (LQRFactory sub-space, control/lqr.py:214-224)"
                       % CTRLR)
    cand = {"controller": "lqr", "finite_horizon": is_finite_horizon(ctrl["finite_horizon"])}
    if cand["finite_horizon"]:
        if "horizon" not in ctrl:
            raise KeyError("finite-horizon LQR configuration has no %s:horizon" % CTRLR)
        cand["horizon"] = int(ctrl["horizon"])
    _cost_and_model(system, cand, cost, model)
    cand["cfg"] = cfg
    return cand


def lqr_candidates_from_configs(system, cfgs):
    return [lqr_candidate_from_config(system, c) for c in cfgs]


def candidates_from_configs(system, cfgs):
    return [candidate_from_config(system, c) for c in cfgs]


def _diagonal(v, n, name):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 2:
        if np.any(v - np.diag(np.diag(v)) != 0.0):
            raise ValueError("%s is not diagonal: QuadCostFactory's configuration space holds diagonal gains only" % name)
        v = np.diag(v)
    if v.shape != (n,):
        raise ValueError("%s has shape %r, expected (%d,)" % (name, v.shape, n))
    return v


def config_from_candidate(system, cand):
    """The pipeline configuration (reference key names) of a candidate: the inverse of candidate_from_config.
    A candidate that came from a configuration returns that configuration."""
    if cand.get("cfg") is not None:
        return cand["cfg"]
    out = DictConfiguration()
    for k, v in (cand.get("model_cfg") or {}).items():
        out["%s:%s" % (MODEL, k)] = v
    if cand.get("controller") == "lqr":
        # LQRFactory's conditional space: horizon is active only under finite_horizon == "true"
        from .lqr_eval import is_finite_horizon
        finite = is_finite_horizon(cand.get("finite_horizon", True))
        out["%s:finite_horizon" % CTRLR] = "true" if finite else "false"
        if finite:
            out["%s:horizon" % CTRLR] = int(cand["horizon"])
    else:
        out["%s:horizon" % CTRLR] = int(cand["horizon"])
    if "num_path" in cand:
        out["%s:sigma" % CTRLR] = float(cand["sigma"])
        out["%s:lmda" % CTRLR] = float(cand["lmda"])
        out["%s:num_path" % CTRLR] = int(cand["num_path"])
    no, nu = system.obs_dim, system.ctrl_dim
    for n, g in zip(system.observations, _diagonal(cand["Q"], no, "Q")):
        out["%s:%s_Q" % (COST, n)] = float(g)
    for n, g in zip(system.observations, _diagonal(cand["F"], no, "F")):
        out["%s:%s_F" % (COST, n)] = float(g)
    for n, g in zip(system.controls, _diagonal(cand["R"], nu, "R")):
        out["%s:%s_R" % (COST, n)] = float(g)
    return out


def sample_mlp_config(rng):
    """One draw from MLPFactory's space (mlp.py:107-135): activation, depth as the STRING the reference's
    categorical holds, the hidden sizes the depth activates (16-256), log-uniform learning rate 1e-5..1."""
    depth = int(rng.integers(1, 5))
    cfg = {"nonlintype": str(rng.choice(["relu", "tanh", "sigmoid", "selu"])), "n_hidden_layers": str(depth)}
    for i in range(depth):
        cfg["hidden_size_%d" % (i + 1)] = int(rng.integers(16, 257))
    cfg["lr"] = float(10 ** rng.uniform(-5, 0))
    return cfg


def sample_pipeline_configs(system, n, rng, controller="mppi", model_axis=False):
    """`n` configurations with the reference's key names, drawn from the factories' ranges: MPPI horizon 5-30,
    sigma 1e-4-2, lmda 0.1-2, num_path 100-1000 (mppi.py:48-64) or iLQR horizon 5-25 (ilqr.py:36-41); cost
    gains log-uniform in [1e-3, 1e4] (quad_cost_factory.py:40-61); with model_axis the MLP sub-space."""
    out = []
    for _ in range(int(n)):
        c = DictConfiguration()
        if model_axis:
            for k, v in sample_mlp_config(rng).items():
                c["%s:%s" % (MODEL, k)] = v
        if controller == "mppi":
            c["%s:horizon" % CTRLR] = int(rng.integers(5, 31))
            c["%s:sigma" % CTRLR] = float(rng.uniform(1e-4, 2.0))
            c["%s:lmda" % CTRLR] = float(rng.uniform(0.1, 2.0))
            c["%s:num_path" % CTRLR] = int(rng.integers(100, 1001))
        elif controller == "ilqr":
            c["%s:horizon" % CTRLR] = int(rng.integers(5, 26))
        else:
            raise ValueError("controller must be 'mppi' or 'ilqr'")
        for name in system.observations:
            c["%s:%s_Q" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        for name in system.observations:
            c["%s:%s_F" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        for name in system.controls:
            c["%s:%s_R" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        out.append(c)
    return out


def sample_arx_config(rng):
    """One draw from ARXFactory's space (arx.py:33-40): history uniform in 1..10."""
    return {"history": int(rng.integers(1, 11))}


def sample_koopman_config(rng, methods=("lstsq", "lasso")):
    """One draw from KoopmanFactory's space (koopman.py:46-77): method, lasso_alpha log-uniform 1e-10..1e2 (method
    lasso), poly_basis / poly_degree 2..8, trig_basis / trig_freq 1..8, product_terms "false"; the conditional keys
    appear only under their parent's value.  The method is drawn from `methods`, by default {lstsq, lasso}: the
    reference's third choice, "stable", is fitted by ``fit_linear_models(..., stable="device")`` (``Koopman.train``
    itself refuses it); ``methods=("lstsq", "lasso", "stable")`` draws from the reference's full space."""
    for m in methods:
        if m not in ("lstsq", "lasso", "stable"):
            raise ValueError("methods must be drawn from lstsq, lasso and stable")
    cfg = {"method": str(rng.choice(list(methods)))}
    if cfg["method"] == "lasso":
        cfg["lasso_alpha"] = float(10 ** rng.uniform(-10, 2))
    cfg["poly_basis"] = str(rng.choice(["true", "false"]))
    if cfg["poly_basis"] == "true":
        cfg["poly_degree"] = int(rng.integers(2, 9))
    cfg["trig_basis"] = str(rng.choice(["true", "false"]))
    if cfg["trig_basis"] == "true":
        cfg["trig_freq"] = int(rng.integers(1, 9))
    cfg["product_terms"] = "false"
    return cfg


def sample_lqr_pipeline_configs(system, n, rng, model=None, koopman_methods=None):
    """`n` (ARX | Koopman) x LQR x QuadCost configurations with the reference's key names: finite_horizon uniform
    over {"true", "false"}, ``_ctrlr:horizon`` (1..1000) only when "true" (lqr.py:214-224), cost gains as
    sample_pipeline_configs; model None (no `_model:` keys), "arx" or "koopman" (that factory's sub-space;
    koopman_methods: the ``methods`` of ``sample_koopman_config``, None for its default)."""
    koopman = sample_koopman_config if koopman_methods is None else (
        lambda r: sample_koopman_config(r, methods=koopman_methods))
    draw = {None: None, "arx": sample_arx_config, "koopman": koopman}
    if model not in draw:
        raise ValueError("model must be None, 'arx' or 'koopman'")
    out = []
    for _ in range(int(n)):
        c = DictConfiguration()
        if draw[model] is not None:
            for k, v in draw[model](rng).items():
                c["%s:%s" % (MODEL, k)] = v
        finite = str(rng.choice(["true", "false"]))
        c["%s:finite_horizon" % CTRLR] = finite
        if finite == "true":
            c["%s:horizon" % CTRLR] = int(rng.integers(1, 1001))
        for name in system.observations:
            c["%s:%s_Q" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        for name in system.observations:
            c["%s:%s_F" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        for name in system.controls:
            c["%s:%s_R" % (COST, name)] = float(10 ** rng.uniform(-3, 4))
        out.append(c)
    return out
