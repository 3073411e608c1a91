"""MI355X-native ResNet-26 + attention-MIL hot path.

Importable as `mil_amd` (repo-root shim `mil_amd.py`); the on-disk package directory keeps the
project's hyphenated name."""
from ._lib import BF16X3, LIB_PATH, MilLibraryError, build_library, lib  # noqa: F401
from . import alt_resnet  # noqa: F401
from .encoder import BasicResBlock, ResNet, invalidate_packed_weights  # noqa: F401
from .dist import FlatAdam, FlatParams, gather_features, shard_bags  # noqa: F401
from .train import BagTrainer, layer_weight_summary_max, layer_weight_summary_mean, load_checkpoint, save_checkpoint, set_stage, stage_for_epoch, visualize_terms, write_attention_map, write_map  # noqa: F401
from .preprocess import S2dTiles, TilePreprocessor, U8Tiles  # noqa: F401
from .roi_select import RoiSelector  # noqa: F401
from .slide_bag import SlideBag  # noqa: F401
from .heatmap import AttentionMapRenderer  # noqa: F401
from .color_jitter import ColorJitter  # noqa: F401
from .stain import HED, StainAffine, StainFit, StainJitter, StainNormalizer  # noqa: F401
from .affine import RandomAffine, affine_matrix, quarter_turn_matrix  # noqa: F401
from .elastic import ElasticDeform  # noqa: F401
from .blur_u8 import GaussianBlurU8, gaussian_blur_u8  # noqa: F401
from .model import Attention, ContextLayer, CrossEntropyWithProbs, TileParallel  # noqa: F401
from .summary import ActivationSummary, parameter_stats, tensor_stats  # noqa: F401
from .saliency import TileSaliency  # noqa: F401
from .gradcam import TileGradCam  # noqa: F401
from .path_attr import TileIntegratedGradients, TileSmoothGrad  # noqa: F401
from .attr_render import AttributionRenderer  # noqa: F401
from .attr_mosaic import AttributionMosaic  # noqa: F401
from .feature_vis import FeatureVisResult, FeatureVisualizer  # noqa: F401
from .feature_inv import FeatureInverter, InversionResult, PixelRegularizer, gaussian_blur  # noqa: F401
from .guided import TileGuidedBackprop, TileGuidedGradCam  # noqa: F401

__all__ = ["alt_resnet", "Attention", "ResNet", "BasicResBlock", "ContextLayer", "CrossEntropyWithProbs", "TileParallel",
           "FlatParams", "FlatAdam", "shard_bags", "gather_features", "BagTrainer", "set_stage", "stage_for_epoch", "write_attention_map", "write_map", "visualize_terms", "save_checkpoint", "load_checkpoint", "TilePreprocessor", "S2dTiles", "U8Tiles", "RoiSelector", "SlideBag", "AttentionMapRenderer", "ColorJitter", "build_library", "lib", "MilLibraryError", "LIB_PATH", "BF16X3", "invalidate_packed_weights",
           "ActivationSummary", "parameter_stats", "tensor_stats", "TileSaliency", "TileGradCam", "TileIntegratedGradients", "TileSmoothGrad", "AttributionRenderer",
           "AttributionMosaic", "FeatureVisualizer", "FeatureVisResult", "FeatureInverter", "InversionResult", "PixelRegularizer", "gaussian_blur",
           "TileGuidedBackprop", "TileGuidedGradCam", "HED", "StainAffine", "StainFit", "StainJitter", "StainNormalizer",
           "RandomAffine", "affine_matrix", "quarter_turn_matrix", "ElasticDeform", "GaussianBlurU8", "gaussian_blur_u8"]
