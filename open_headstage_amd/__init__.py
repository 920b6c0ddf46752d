"""open_headstage_amd -- MI355X-native binaural convolution core.

Drop-in for the `src/dsp` hot path of KiloHertzian/Open-Headstage (4-path HRIR
partitioned FFT convolution + 10-band parametric EQ), as hand-written gfx950 HIP
kernels behind the C ABI in include/ohs_hip.h.  This package is the host-side
mirror of the reference's Rust interface plus the many-stream batch mode; it
contains no CPU compute path.
"""
from .dsp import (BLOCK_SIZE, FFT_SIZE, NUM_EQ_BANDS, BandConfig, BiquadFilter, ConvolutionEngine, ConvolutionPath,
                  FilterType, StereoParametricEQ, biquad_coefficients, process_chain)
from .batch import LAYOUT_5_1, LAYOUT_7_1, BatchProcessor, NodeBatchProcessor
from .session import HeadTrack, SessionRenderer, nearest_set, plan_calls, render_files, yaw_rows
from .pcm import WavReader, pcm_decode_device, pcm_encode_device
from .autoeq import BandSetting, apply_bands, parse_autoeq_csv, parse_autoeq_csv_text
from .scene import SceneError, SceneProcessor, nearest_directions, rotate_sources
from .scene2 import BlendSceneProcessor, bracket_directions
from .scene3 import TriSceneProcessor, triangle_directions, triangulate_directions
from .lookup import DirectionLookup, DirectionLookupError
from .lookup3 import TriangleLookup, TriangleLookupError
from .lookup3p import PrunedTriangleLookup, PrunedTriangleLookupError
from .tracked import TrackedSceneProcessor
from .delay import ObjectDelay, ObjectDelayError, distance_rows, render_with_distance
from .delay2 import FilteredObjectDelay, FilteredObjectDelayError, air_absorption_taps, render_with_distance_air
from ._ffi import OhsError

__all__ = ["BLOCK_SIZE", "FFT_SIZE", "NUM_EQ_BANDS", "BandConfig", "BiquadFilter", "ConvolutionEngine",
           "ConvolutionPath", "FilterType", "StereoParametricEQ", "biquad_coefficients",
           "process_chain", "BatchProcessor", "NodeBatchProcessor", "OhsError", "BandSetting", "apply_bands",
           "parse_autoeq_csv", "parse_autoeq_csv_text", "LAYOUT_5_1", "LAYOUT_7_1", "SessionRenderer",
           "HeadTrack", "nearest_set", "yaw_rows", "plan_calls", "render_files", "WavReader", "pcm_decode_device",
           "pcm_encode_device", "SceneProcessor", "SceneError", "rotate_sources", "nearest_directions",
           "BlendSceneProcessor", "bracket_directions", "TriSceneProcessor", "triangle_directions",
           "triangulate_directions", "DirectionLookup", "DirectionLookupError", "TriangleLookup",
           "TriangleLookupError", "PrunedTriangleLookup", "PrunedTriangleLookupError",
           "TrackedSceneProcessor", "ObjectDelay", "ObjectDelayError", "distance_rows", "render_with_distance",
           "FilteredObjectDelay", "FilteredObjectDelayError", "air_absorption_taps", "render_with_distance_air"]
