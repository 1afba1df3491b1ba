"""String constants (same vocabulary as the reference's diffmusic/constants.py:1-35)."""
CONFIG_PATH = "configs"
MOISES, MUSICCAPS = "moises", "music_data"
AUDIOLDM2, MUSICLDM = "audioldm2", "musicldm"
MUSIC_GENERATION, MUSIC_INPAINTING, SUPER_RESOLUTION = "music_generation", "music_inpainting", "super_resolution"
PHASE_RETREVAL, MUSIC_DEREVERBERATION, STYLE_GUIDANCE = "phase_retrieval", "music_dereverberation", "style_guidance"
MUSIC_DECLIPPING = "music_declipping"          # extension: hard clipping (inverse_problem/operator.py DeclippingOperator)
MUSIC_BLIND_DEREVERBERATION = "music_blind_dereverberation"   # extension: unknown response (BlindDereverberationOperator)
MUSIC_SOURCE_SEPARATION = "music_source_separation"           # extension: stems of a mixture (inverse_problem/mixture.py MixtureOperator)
MUSIC_SPECTRAL_INPAINTING = "music_spectral_inpainting"       # extension: a gain on a region of the spectrogram (TimeFrequencyMaskOperator)
MUSIC_BLIND_EQUALIZATION = "music_blind_equalization"         # extension: an unknown EQ curve, fitted (BlindEqualizationOperator)
MUSIC_DECOMPRESSION = "music_decompression"                   # extension: dynamic-range compression undone (DynamicRangeOperator)
MUSIC_WOW_FLUTTER = "music_wow_flutter"                       # extension: a varying playback speed undone (TimeWarpOperator)
MUSIC_BLIND_WOW_FLUTTER = "music_blind_wow_flutter"           # extension: an unknown delay curve, fitted (BlindTimeWarpOperator)
MUSIC_BLIND_DECOMPRESSION = "music_blind_decompression"       # extension: unknown compressor settings, fitted (BlindDynamicRangeOperator)
DDIM, DPS, MPGD, DSG, DITTO, DIFFMUSIC = "ddim", "dps", "mpgd", "dsg", "ditto", "diffmusic"
NULL_TEXT, TAG, CLAP = "null_text", "tag", "clap"
WAV_FORM, MEL_SPECTROGRAM = "wav_form", "mel_spectrogram"
