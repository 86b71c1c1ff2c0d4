"""tiresias_amd — MI355X-native fingerprint engine for asterisk-tiresias (Python side).

The compute lives in lib/libtiresias_fp.so (HIP, gfx950) behind include/tiresias_fp.h;
this package is its ctypes binding plus a mirror of the reference's fp_handler interface.
"""
from ._lib import LIB_PATH, NULL_MICRO, TfpError, header_symbols, lib  # noqa: F401
from .engine import (ALAW, FRAME_DTYPE, MIX_CHANNELS_MAX, ULAW, Engine, Group, GroupLive, GroupStream, Live, Plan, Stream, census_at_least,  # noqa: F401
                     decode_g711, decode_wav_g711, decode_wav_interleaved, device_count, frame_count, params, read_wav_g711, read_wav_interleaved, resample_count, resample_mix_pcm, resample_pcm,
                     resample_taps, sliding_windows, synth_pcm)
from .engine import decode_wav_interleaved_q31, q31_from_float, read_wav_interleaved_q31, resample_wide_pcm  # noqa: F401
from .engine import (ANY_RATES_MAX, AUDIO_ALAW, AUDIO_Q31, AUDIO_S16, AUDIO_ULAW, CLIP_DTYPE, audio_clips_check,  # noqa: F401
                     pack_audio_clips, resample_any_pcm)
from .fp_handler import FpHandler  # noqa: F401
