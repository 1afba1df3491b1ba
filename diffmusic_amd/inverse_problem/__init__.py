from .noise import GaussianNoise, PoissonNoise
from .operator import (BaseOperator, IdentityOperator, MusicInpaintingOperator, PhaseRetrievalOperator,
                       SuperResolutionOperator, MusicDereverberationOperator, StyleGuidanceOperator, DeclippingOperator,
                       TimeFrequencyMaskOperator, DynamicRangeOperator, TimeWarpOperator, DeclickOperator, CodecOperator)
from .blind import BlindDereverberationOperator, BlindEqualizationOperator, BlindTimeWarpOperator, BlindDynamicRangeOperator
from .dsp import click_train, threshold_for_sdr, tf_frames, tf_gain_grid, hum_boxes, eq_curve, lowpass_curve, drc_coeffs, drc_static_curve, \
    warp_knots, wow_curve, check_warp_curve, warp_coarse_knots, warp_expand, drc_table, drc_time_ms, mdct_frames, mdct, imdct, codec_bands, \
    codec_step_grid, codec_steps_for_nmr
from .track import TrackLayout, TrackOperator, seconds_for_samples
from .mixture import MixtureOperator


def get_noiser(name, sigma, stream="global"):  # reference: inverse_problem/__init__.py:4-11; `stream`: GaussianNoise's per-step stream
    if name == "gaussian":
        return GaussianNoise(sigma, stream=stream)
    if name == "poisson":
        return PoissonNoise(sigma)
    raise ValueError(f"Unknown noise: {name}")
