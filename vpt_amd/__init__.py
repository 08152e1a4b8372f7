"""vpt_amd — MI355X-native re-host of the MIP / EAM / MCS / MCM renderer path of MOj0/vpt.

Host-side mirror of the reference's Renderer plugin surface over a C-ABI HIP library
(include/vpt.h -> vpt_amd/libvpt_hip.so).  Importing the package does not load the library;
constructing a Context does, and raises if it is missing (no CPU fallback)."""
from .property_bag import PropertyBag, EventTarget, Event, CustomEvent
from .scene import Node, Transform, PerspectiveCamera, mat4, quat, vec3, default_camera, mvp_inverse_matrix
from .context import Context
from .volume import Volume, Components, Distance, Skeleton, Surface, Graph
from .loaders import AbstractLoader, BlobLoader, FileLoader, LoaderFactory
from .readers import AbstractReader, RAWReader, ZIPReader, BVPReader, ReaderFactory
from .renderers import (AbstractRenderer, MIPRenderer, EAMRenderer, MCSRenderer, MCMRenderer, ISORenderer, DepthRenderer, LAORenderer, DOSRenderer,
                        RendererFactory)
from .tonemappers import (AbstractToneMapper, ArtisticToneMapper, RangeToneMapper, ReinhardToneMapper, Reinhard2ToneMapper,
                          Uncharted2ToneMapper, FilmicToneMapper, UnrealToneMapper, AcesToneMapper, LottesToneMapper,
                          UchimuraToneMapper, ToneMapperFactory)
from .rendering_context import RenderingContext
from .animators import CircleAnimator, OrbitCameraAnimator
from .transfer_function import TransferFunction
from .hdr import HDRImage, read_hdr
from .gradient import gradient_magnitude
from .window import window_texels, percentile_window
from .pyramid import reduce_texels, smooth_texels
from .rank import rank_texels
from .components import components_texels, keep_texels, label_texels
from .measure import measure_texels, keep_set_texels, derive, MEASURE_DTYPE
from .distance import distance_squared_texels, within_texels, channel_texels, check_seeds, check_steps, check_radius
from .distance import thickness_squared_texels, thickness_texels, open_ball_texels
from .skeleton import skeleton_burn_texels, skeleton_texels, burn_within_texels, check_skeleton
from .graph import graph_texels, skeleton_graph_texels, prune_texels, classes_texels, centreline_texels, BRANCH_DTYPE, NODE_DTYPE
from .surface import surface_texels, write_stl, write_ply, write_obj
from .resample import resample_texels, isotropic_shape, axis_taps, nearest_index, count_ties, check_mode, check_size, check_spacing
from .combine import combine_texels, compare_stats, OPS, check_op, check_weights, check_channel
from .reconstruct import reconstruct_texels, geodesic_texels, RECONSTRUCT_OPS, GEODESIC_OPS
from .watershed import watershed_texels, descent_texels, split_texels, POLARITIES, check_polarity, check_split
from ._native import VptError

__all__ = [
    'PropertyBag', 'EventTarget', 'Event', 'CustomEvent', 'Node', 'Transform', 'PerspectiveCamera',
    'mat4', 'quat', 'vec3', 'default_camera', 'mvp_inverse_matrix', 'Context', 'Volume', 'RAWReader',
    'AbstractLoader', 'BlobLoader', 'FileLoader', 'LoaderFactory', 'AbstractReader', 'ZIPReader', 'BVPReader', 'ReaderFactory',
    'AbstractRenderer', 'MIPRenderer', 'EAMRenderer', 'MCSRenderer', 'MCMRenderer', 'ISORenderer', 'DepthRenderer', 'LAORenderer', 'DOSRenderer', 'RendererFactory', 'VptError',
    'AbstractToneMapper', 'ArtisticToneMapper', 'RangeToneMapper', 'ReinhardToneMapper', 'Reinhard2ToneMapper',
    'Uncharted2ToneMapper', 'FilmicToneMapper', 'UnrealToneMapper', 'AcesToneMapper', 'LottesToneMapper',
    'UchimuraToneMapper', 'ToneMapperFactory', 'RenderingContext', 'CircleAnimator', 'OrbitCameraAnimator', 'TransferFunction',
    'HDRImage', 'read_hdr', 'gradient_magnitude', 'window_texels', 'percentile_window', 'reduce_texels', 'smooth_texels', 'rank_texels',
    'components_texels', 'keep_texels', 'label_texels', 'Components',
    'measure_texels', 'keep_set_texels', 'derive', 'MEASURE_DTYPE',
    'distance_squared_texels', 'within_texels', 'channel_texels', 'check_seeds', 'check_steps', 'check_radius', 'Distance',
    'thickness_squared_texels', 'thickness_texels', 'open_ball_texels',
    'skeleton_burn_texels', 'skeleton_texels', 'burn_within_texels', 'check_skeleton', 'Skeleton',
    'graph_texels', 'skeleton_graph_texels', 'prune_texels', 'classes_texels', 'centreline_texels', 'BRANCH_DTYPE', 'NODE_DTYPE', 'Graph',
    'surface_texels', 'write_stl', 'write_ply', 'write_obj', 'Surface',
    'resample_texels', 'isotropic_shape', 'axis_taps', 'nearest_index', 'count_ties', 'check_mode', 'check_size', 'check_spacing',
    'combine_texels', 'compare_stats', 'OPS', 'check_op', 'check_weights', 'check_channel',
    'reconstruct_texels', 'geodesic_texels', 'RECONSTRUCT_OPS', 'GEODESIC_OPS',
    'watershed_texels', 'descent_texels', 'split_texels', 'POLARITIES', 'check_polarity', 'check_split',
]
