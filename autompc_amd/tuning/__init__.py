from .batch_eval import (CandidateEvaluator, IlqrCandidateEvaluator, balanced_shards, candidate_work,
                         evaluate_sharded, random_candidates, random_ilqr_candidates, score_trajectories,
                         shard_bounds)
from .lqr_eval import LqrCandidateEvaluator, random_lqr_candidates
from .batch_tuner import BatchPipelineTuner, PipelineTuneResult
from .model_tuner import BatchModelTuner, ModelTuneResult
from .proposer import CandidateEncoder, GpProposer, gp_propose_host
from .configs import (DictConfiguration, candidate_from_config, candidates_from_configs, config_from_candidate,
                      lqr_candidate_from_config, sample_arx_config, sample_koopman_config,
                      sample_lqr_pipeline_configs, sample_pipeline_configs)

__all__ = ["CandidateEvaluator", "IlqrCandidateEvaluator", "balanced_shards", "candidate_work", "evaluate_sharded", "random_candidates",
           "random_ilqr_candidates", "score_trajectories", "shard_bounds", "BatchPipelineTuner",
           "PipelineTuneResult", "DictConfiguration", "candidate_from_config", "candidates_from_configs",
           "config_from_candidate", "sample_pipeline_configs", "BatchModelTuner", "ModelTuneResult",
           "LqrCandidateEvaluator", "random_lqr_candidates", "lqr_candidate_from_config", "sample_arx_config",
           "sample_koopman_config", "sample_lqr_pipeline_configs", "CandidateEncoder", "GpProposer", "gp_propose_host"]
