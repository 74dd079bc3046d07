"""``src.models`` of the reference (``src/models.py:7-193``) served by the HIP path."""
from robust_speech_analysis_framework_amd.cnnlstm import (  # noqa: F401
    AttentionPooling, CNNLSTM, CNNLSTMGroup, FusedAdam, ResidualBlock, cnnlstm_forward_group, cnnlstm_train_group,
    cnnlstm_train_step_group, eval_model_grouped, eval_replicas_lockstep, get_activation_fn,
    train_eval_replicas_lockstep, train_replicas_lockstep)
from robust_speech_analysis_framework_amd.layer_mix import LayerMix  # noqa: F401
from robust_speech_analysis_framework_amd.layer_mix_train import cnnlstm_mix_train_step_group, collate_mix_batches  # noqa: F401
