"""fs2amd — MI355X-native FastSpeech2 mel-synthesis forward (HIP/CDNA4 kernels behind a C ABI).

    from fs2amd import FastSpeech2          # drop-in for the reference model/fastspeech2.py
    from fs2amd import TacotronSTFT         # drop-in for the reference audio/stft.py (mel / energy targets)
"""
from .align import AlignmentEncoder, ForwardSumLoss, fit_aligner, mas_durations
from .augment import augment_utterances, pitch_shift, time_stretch
from .audio import (STFT, TacotronSTFT, extract_features, get_mel_from_wav, griffin_lim, inv_mel_spec, mel_filterbank,
                    mel_to_wav, window_sumsquare)
from .emotion import curve, level_weights, mixture, one_hot
from .evaluate import dtw, evaluate, f0_metrics, mcd, mel_cepstrum
from .loss import FastSpeech2Loss
from .loudness import integrated_loudness, normalize_loudness
from .model import FastSpeech2, LengthRegulator
from .optimizer import ScheduledOptim
from .preprocess import (CorpusStats, build_corpus, f0_contour, get_alignment, normalize, pitch_targets,
                         prepare_wavs, remove_outlier, split_silence, trim_silence)

__all__ = ["FastSpeech2", "FastSpeech2Loss", "ScheduledOptim", "LengthRegulator", "TacotronSTFT",
           "get_mel_from_wav", "extract_features", "mel_filterbank", "STFT", "griffin_lim", "inv_mel_spec",
           "mel_to_wav", "window_sumsquare", "get_alignment", "pitch_targets", "remove_outlier", "CorpusStats",
           "normalize", "build_corpus", "f0_contour", "prepare_wavs", "ForwardSumLoss", "AlignmentEncoder",
           "mas_durations", "fit_aligner", "trim_silence", "split_silence", "time_stretch", "pitch_shift",
           "augment_utterances", "integrated_loudness", "normalize_loudness", "mixture", "level_weights",
           "curve", "one_hot", "mcd", "dtw", "mel_cepstrum",
           "f0_metrics", "evaluate"]
