"""ishara_amd — MI355X-native (gfx950) hot path of the Ishara ASL-fingerspelling recogniser:
the Conv1D -> Squeezeformer -> Conformer CTC encoder behind the reference's get_model(...) /
model.fit surface.  See DESIGN.md and include/ishara_hip.h."""
from .model import (Callback, History, LearningRateScheduler, Model, Optimizer, PAD_TOKEN_IDX,  # noqa: F401
                    frame_lengths, get_model, lrfn, make_config)
from ._lib import IsharaError  # noqa: F401
from .conformer import ConformerEncoder  # noqa: F401  (torch family: conformer/conformer.py)
from .squeezeformer import Squeezeformer, SqueezeformerEncoder  # noqa: F401  (torch family: squeezeformer/encoder.py, model.py)
from .tflite_batch import BatchedTFLiteModel  # noqa: F401  (batched raw-clip inference + device test-set scoring)
from .tflite_stream import StreamingTFLiteModel, StreamReference, StreamResult  # noqa: F401  (streaming sessions: stable prefix, endpointing)
from .ctc_beam import CharBigramLM, prefix_beam_search  # noqa: F401  (CTC prefix beam search: host reference, bigram LM)
from .ctc_lm import CharNGramLM, LMAutomaton  # noqa: F401  (character n-gram LMs as automata, for the beam search's lm=)
from . import ctc_align  # noqa: F401  (forced alignment: the module, callable as ctc_align(logits, labels, lengths))
from .ctc import ctc_beam_decode, ctc_greedy_decode, ctc_loss  # noqa: F401  (CTC with per-clip frame counts)
from .score import edit_alignment_device  # noqa: F401  (edit-operation alignment of device decodes: ops, positions, confusion matrix)
from .ensemble import EnsembleTFLiteModel, combine_logits, combine_reference, normalise_weights  # noqa: F401  (model ensembling: device logit fusion)
from .mbr import mbr_reference, mbr_select, pool_nbest  # noqa: F401  (minimum-Bayes-risk decoding over the beam's n-best)
from .rescore import (ctc_logp_reference, ctc_score_nbest, rescore_models, rescore_nbest,  # noqa: F401  (second-pass n-best rescoring:
                      rescore_reference)                                                   # exact CTC scores, LM, rerank)
from .rescore import rescore_sweep, rescore_sweep_reference, sweep_grid, sweep_scores  # noqa: F401  (its weight sweep on the device)
from .mwer import ctc_nbest_grad, mwer_loss, mwer_reference, mwer_weights  # noqa: F401  (minimum-risk training over the beam's n-best)
from .kd import kd_grad, kd_loss, kd_reference  # noqa: F401  (knowledge distillation from a teacher's frame posteriors)
