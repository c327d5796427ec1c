"""Public names of the vti_amd package."""
from ._lib import LIB_PATH, SIGNATURES, VtiError, lib
from .engine import Engine, FrameTable, WindowTable, NmsParams, NmsTable, RawTable, StampTable, debug_conv2d, debug_decode, debug_sppf_pool, debug_upsample2x, h2_decode, h2_encode, kmeans1d2, pixels_to_world, unpack_bits
from .feeder import FrameFeeder
from .model import YOLO, Boxes, Masks, RawFrames, Results, letterbox_shape
from .weights import pack_container, random_weights, unpack_container
from .convert import convert_checkpoint, convert_state_dict
from .measure import CheckerParams, MeasureParams, MultiCameraChecker, MultiCameraMeasurer, StitchDistanceChecker, StitchMeasurer, checker_text_items
from .annotate import checker_display_list
from . import annotate, consumer, dataparallel, jpeg, overlay, rawframes

__all__ = ["LIB_PATH", "SIGNATURES", "VtiError", "lib", "Engine", "FrameTable", "WindowTable", "NmsParams", "NmsTable", "RawTable", "StampTable", "debug_conv2d", "debug_decode", "debug_sppf_pool", "debug_upsample2x", "h2_decode", "h2_encode", "kmeans1d2", "pixels_to_world", "unpack_bits", "FrameFeeder", "YOLO", "Boxes", "Masks", "RawFrames",
           "Results", "letterbox_shape", "pack_container", "random_weights", "unpack_container", "convert_checkpoint", "convert_state_dict",
           "MeasureParams", "MultiCameraMeasurer", "StitchMeasurer", "CheckerParams", "StitchDistanceChecker", "MultiCameraChecker", "checker_text_items", "checker_display_list", "annotate", "consumer", "dataparallel", "jpeg", "overlay", "rawframes"]
