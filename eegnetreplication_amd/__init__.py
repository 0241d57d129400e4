"""MI355X-native EEGNet train/infer step (drop-in for PraKesEy/EEGNetReplication's hot path).

Public surface mirrors ``eegnet_repl.model``: ``EEGNet``, ``train``, ``evaluate_model``; ``saliency``
and ``relevance_maps`` give the eval-mode input gradients the reference gets from plain autograd;
``sliding_logits``, ``cropped_predict`` and ``evaluate_cropped`` classify every window of a continuous
recording in place and ``epoch_logits`` the windows a cue table places (``epoch_starts``), on which
``finetune_on_recording`` fine-tunes a frozen-BatchNorm model without copying them out; ``design_bandpass``,
``bandpass_filter`` / ``StreamBandpass`` and ``exponential_moving_standardize`` / ``StreamStandardizer``
(together: ``preprocess_recording``) band-pass and standardise a raw recording for them on the device, as the
reference's preprocessing does, and ``resample`` / ``resample_to`` / ``StreamResampler`` (``design_resampler``,
``resampled_length``, ``resampled_onsets``, ``resample_ratio``) bring it to the model's rate first -- by the
polyphase method, not by the FFT method the reference's ``raw.resample`` defaults to.
The compute runs in ``libeegnet_hip.so`` (hand-written gfx950 HIP kernels, C-ABI in
``include/eegnet_abi.h``).
"""

from .model import EEGNet, FusedTrainer, evaluate_model, relevance_maps, saliency, train  # noqa: F401
from .model import cropped_predict, evaluate_cropped, sliding_logits, window_starts  # noqa: F401
from .folds import FoldBatch, FrozenFoldBatch, evaluate_folds  # noqa: F401
from .ops import Shape  # noqa: F401
from .model import epoch_logits, epoch_starts, finetune_on_recording  # noqa: F401
from .preprocess import StreamStandardizer, exponential_moving_standardize  # noqa: F401
from .preprocess import StreamBandpass, bandpass_filter, design_bandpass, preprocess_recording  # noqa: F401
from .preprocess import StreamResampler, design_resampler, resample, resample_ratio, resample_to  # noqa: F401
from .preprocess import resampled_length, resampled_onsets  # noqa: F401

__all__ = ["EEGNet", "FoldBatch", "FrozenFoldBatch", "FusedTrainer", "Shape", "StreamBandpass", "StreamResampler",
           "StreamStandardizer", "bandpass_filter", "cropped_predict", "design_bandpass", "design_resampler",
           "epoch_logits", "epoch_starts", "evaluate_cropped", "evaluate_folds", "evaluate_model",
           "exponential_moving_standardize", "finetune_on_recording", "preprocess_recording", "relevance_maps", "resample", "resample_ratio",
           "resample_to", "resampled_length", "resampled_onsets", "saliency", "sliding_logits", "train",
           "window_starts"]
