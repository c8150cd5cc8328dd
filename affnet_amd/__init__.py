"""affnet_amd - MI355X-native implementation of the ScaleSpaceAffinePatchExtractor hot path of
ducha-aiki/affnet behind the reference's Python API.  All device work lives in
libaffnet_hip.so (affnet_amd/csrc, C ABI in include/affnet_hip.h); importing this package
fails loudly if the library has not been built."""
from . import _lib  # noqa: F401  (raises ImportError when libaffnet_hip.so is missing)
from .SparseImgRepresenter import ScaleSpaceAffinePatchExtractor, get_geometry_and_descriptors  # noqa: F401
from .architectures import AffNetFast, OriNetFast, AffNetFastFullConv  # noqa: F401
from .OnePassSIR import OnePassSIR  # noqa: F401
from .HardNet import HardNet, HardTFeatNet  # noqa: F401
from .pytorch_sift import SIFTNet  # noqa: F401
from . import LAF, HandCraftedModules, Losses, ReprojectionStuff, pytorch_sift  # noqa: F401
from .ReprojectionStuff import verify_matches, enqueue_verify, match_and_verify  # noqa: F401
from .ReprojectionStuff import verify_epipolar, enqueue_verify_epipolar, sampson_distance  # noqa: F401
from .ReprojectionStuff import verify_epipolar_planar, enqueue_verify_epipolar_planar  # noqa: F401
from .ReprojectionStuff import enqueue_match_guided, match_guided, guided_mask, match_verify_guided  # noqa: F401
from .ReprojectionStuff import enqueue_match_ratio, match_ratio, match_fginn  # noqa: F401
from .ReprojectionStuff import pair_table, enqueue_match_and_verify_many, match_and_verify_many, spatial_rerank  # noqa: F401
from .ReprojectionStuff import enqueue_match_verify_guided_many, match_verify_guided_many  # noqa: F401
from . import retrieval  # noqa: F401
from .retrieval import knn, DescriptorIndex  # noqa: F401
from .retrieval import quantization_scale, quantize, knn_q8, QuantizedDescriptorIndex  # noqa: F401
from .retrieval import train_cells, ivf_layout, ivf_knn, IVFParts, IVFDescriptorIndex  # noqa: F401
from .retrieval import ivf_knn_q8, IVFQ8Parts, IVFQuantizedDescriptorIndex  # noqa: F401
from .synthetic import synthetic_image, synthetic_hardnet_state  # noqa: F401

__version__ = "0.1.0"
