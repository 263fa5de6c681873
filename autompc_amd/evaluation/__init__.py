from .evaluator import ModelEvaluator
from .holdout_evaluator import HoldoutModelEvaluator
from .model_metrics import get_model_rmse, get_model_rmsmens, model_errors

__all__ = ["ModelEvaluator", "HoldoutModelEvaluator", "get_model_rmse", "get_model_rmsmens", "model_errors"]
