"""scattennet_amd — MI355X-native (gfx950 / CDNA4) implementation of the SCAttenNet
spatial-coordinate-attention hot path (tinh2044/SCAttenNet: model/attention.py,
model/keypoint_module.py, model/fusion.py and their helpers).

Drop-in modules keep the reference constructors, forward signatures and state_dict keys;
their math runs in hand-written HIP kernels (libscatten_hip.so, C ABI in include/scatten.h).
"""
from .encoder import SCAEncoder  # noqa: F401
from .fusion import CoordinatesFusion, InvertedResidual  # noqa: F401
from .attention import BaseAttention, CrossAttention, SelfAttention, SelfCausalAttention  # noqa: F401
from .keypoint_module import (CoordinateAttention, CoordinatesMerge, KeypointModule, KeypointStreams,  # noqa: F401
                              SeparativeCoordinateAttention)
from .layers import CoordinateMapping, FeedForward, LearningPositionEmbedding  # noqa: F401
from .residual import ResidualBlock, ResidualNetwork  # noqa: F401
from .data import JointParts, collate_keypoints, normalize_keypoints  # noqa: F401
from .alignment import AlignmentModule  # noqa: F401
from .heads import RecognitionHead, SeqKD, compute_loss, distillation_loss  # noqa: F401
from .decode import (ctc_decode, ctc_decode_device, ctc_greedy_decode_device, decode_outputs, wer_counts,  # noqa: F401
                     wer_from_counts)
from .align import (align_outputs, alignment_lists, ctc_align, ctc_align_device,  # noqa: F401
                    ctc_align_heads_device)
from .optim import FusedAdam, WarmupCosineAnnealingScheduler, build_optimizer, clip_grad_norm_  # noqa: F401
from .model import MSCA_Net, finite_flags, first_error  # noqa: F401
from .train import read_report, train_step  # noqa: F401
from .bucketed import BucketedStep, BucketedTrainStep, pad_batch  # noqa: F401
from .ensemble import EnsembleLogProbsOp, EnsembleSpec, LearnedEnsemble, LearnedEnsembleLogProbsOp  # noqa: F401
from .ensemble import ensemble_log_probs  # noqa: F401
from .distill import Distill, EnsembleDistillOp, check_distill, ensemble_distillation_loss  # noqa: F401
from .mwer import MWER, MWERLossOp, mwer_guard, mwer_loss  # noqa: F401
from .nbest import (BigramLM, NBest, Rescoring, ctc_decode_fused_nbest, ctc_decode_fused_nbest_device,  # noqa: F401
                    ctc_decode_fused_nbest_heads_device, ctc_decode_nbest, ctc_decode_nbest_device,
                    ctc_decode_nbest_heads_device, mbr_select_device, rescore_nbest_device, rescored_decode,
                    select_device)
from .ngram import NGramLM  # noqa: F401
from .evaluate import BucketedEvalStep, EvalState, ctc_decode_heads_device, eval_step  # noqa: F401
from .recognize import BucketedRecognizer, Recognition, recognize_step  # noqa: F401
from . import library  # noqa: F401  (torch.ops.scatten.*)
from .utils import KeyPaddingMask, create_attention_mask, create_causal_attention_mask, key_padding_mask  # noqa: F401

__version__ = "0.1.0"
