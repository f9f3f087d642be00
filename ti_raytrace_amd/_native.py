"""ctypes binding of libtirt.so (the HIP library; C-ABI in include/tirt.h).

There is no CPU fallback: if the library is missing, or no HIP device can be opened, the
calls raise.  (The CPU oracle under oracle/ is test infrastructure and is never loaded
from here.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TIRT_LIB_PATH") or os.path.join(_HERE, "csrc", "libtirt.so")      # (TIRT_LIB_PATH: A/B builds of the same library, tools/ab*.sh)

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class TirtError(RuntimeError):
    pass


class TirtStackOverflow(TirtError):
    """tirt_stats found rays whose traversal stack overflowed (TIRT_ERR_STACK): subtrees were dropped, the
    rendered result is wrong -- raise `stack_size`.  `.stats` holds the statistics that were read."""

    def __init__(self, msg, stats):
        TirtError.__init__(self, msg)
        self.stats = stats


ERR_STACK = -4


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rays_closest", "rays_shadow", "box_closest", "leaf_closest", "box_shadow",
        "leaf_shadow", "shaded", "paths", "stack_overflow")] + [
        (n, C.c_double) for n in ("ms_build", "ms_render", "ms_trace_closest",
                                  "ms_trace_shadow", "ms_shade")] + [
        (n, C.c_uint64) for n in ("launches_trace_closest", "launches_trace_shadow",
                                  "launches_shade", "diag_it_node", "diag_lanes_node", "diag_it_leaf",
                                  "diag_lanes_leaf", "diag_refills", "diag_it_outer", "diag_wave_ticks", "diag_drain_ticks", "diag_waves", "launches_tail")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the counts of tirt_signed_distance_prepare, in its order
SD_REPORT = ("boundary_edges", "nonmanifold_edges", "flipped_edges", "invalid_triangles", "primitives")

TRAVERSE_ORDERED = 0
TRAVERSE_EXHAUSTIVE = 1
COUNT_NODES = 2
PAIRS_COUNT, PAIRS_FILL, PAIRS_BOTH = 0, 1, 2                       # TIRT_PAIRS_*: the modes of tirt_query_point_pairs / tirt_query_mesh_pairs
PAIRS_UNORDERED = 4                                                 # TIRT_PAIRS_UNORDERED: their flag beside the two above

# tirt_debug_render modes (include/tirt.h): the views of integrator/Debug.py:62-65
DEBUG_ALBEDO = 0
DEBUG_FNORMAL = 1
DEBUG_NORMAL = 2
DEBUG_GNORMAL = 3

# the words of a pixel's feature-buffer record (include/tirt.h, TIRT_AOV_*)
AOV_WORDS = 8
AOV_ALBEDO = 0
AOV_NORMAL = 3
AOV_DEPTH = 6
AOV_ALPHA = 7

# the words of a pixel's sample-moment record (include/tirt.h, TIRT_MOM_*)
MOM_WORDS = 8
MOM_N = 0
MOM_MEAN = 1
MOM_M2 = 4
MOM_BAD = 7

# the words of a pixel's motion record (include/tirt.h, TIRT_MOTION_WORDS): D3, 1, dN3, 0
MOTION_WORDS = 8

# bits of the scene feature word (include/tirt.h, tirt_shade_features)
SF_GLASS, SF_ENV, SF_LIGHT_TRI, SF_LIGHT_SPOT_LASER, SF_NO_LIGHT, SF_LIGHT_SPHERE, SF_LIGHT_OTHER = 1, 2, 4, 8, 16, 32, 64
SF_ALL = 127
SF_TEXTURE = 128                                                    # a textured material (tirt_texture_upload); not part of SF_ALL
# the feature words k_shade is compiled for, narrowest first, up to the albedo instantiation (k_shade_spec: the first three); k_shade's fifth and last,
# behind these, is SHADE_INSTANTIATION_MAPS below -- kept out of this tuple, whose last entry the albedo tests hold to 255
SHADE_INSTANTIATIONS = (SF_LIGHT_SPHERE, SF_LIGHT_TRI, SF_ALL, SF_ALL | SF_TEXTURE)
SF_TEXTURE_PARAM = 256                                              # a roughness, metallic or normal-map texture on a material (row words 7..9); not part of SF_ALL
SHADE_INSTANTIATION_MAPS = SF_ALL | SF_TEXTURE | SF_TEXTURE_PARAM   # k_shade's fifth instantiation, behind the four above (that tuple ends at 255: tests/test_texture_abi.py)
SF_CUTOUT = 512                                                     # a cut-out triangle exists (tirt_texture_cutout); reported only: no instantiation of k_shade depends on it
SF_ENV_SAMPLE = 1024                                                # environment importance sampling on, environment lit, table built (tirt_env_sampling); not part of SF_ALL
SHADE_INSTANTIATIONS_ENV = (SF_ALL | SF_ENV_SAMPLE, SHADE_INSTANTIATION_MAPS | SF_ENV_SAMPLE)       # k_shade's twins with the environment's light sample
SF_ENV_HDR = 2048                                                   # the uploaded environment is RGBE8 (tirt_env_upload_hdr) and lit; not part of SF_ALL
SHADE_INSTANTIATIONS_HDR = (SF_ALL | SF_ENV_HDR, SHADE_INSTANTIATION_MAPS | SF_ENV_HDR,             # k_shade's twins that decode RGBE8 texels, without and with the light sample
                            SF_ALL | SF_ENV_SAMPLE | SF_ENV_HDR, SHADE_INSTANTIATION_MAPS | SF_ENV_SAMPLE | SF_ENV_HDR)
ENV_FORMAT_RGB8, ENV_FORMAT_RGBE8 = 0, 1                            # tirt_env_format, Texture.format
KAT_ENV_LOOKUP_IN, KAT_ENV_LOOKUP_OUT = 2, 3                        # words per row of tirt_kat_env_lookup
SF_LIGHT_POWER = 4096                                               # emitters chosen by power, table built with a weight in it (tirt_light_sampling); not part of SF_ALL
SHADE_INSTANTIATIONS_POWER = tuple(f | 4096 for f in (127, 511, 127 | 1024, 511 | 1024, 127 | 2048, 511 | 2048, 127 | 1024 | 2048, 511 | 1024 | 2048))      # k_shade's twins that choose by power
KAT_LIGHT_PICK_IN, KAT_LIGHT_PICK_OUT = 1, 2                        # words per row of tirt_kat_light_pick
KAT_ENV_SAMPLE_IN, KAT_ENV_SAMPLE_OUT = 2, 10                       # words per row of tirt_kat_env_sample
KAT_ENV_PDF_IN, KAT_ENV_PDF_OUT = 3, 5                              # words per row of tirt_kat_env_pdf
KAT_ALPHA_IN, KAT_ALPHA_OUT = 3, 2                                  # words per row of tirt_kat_texture_alpha
KAT_MAPS_IN, KAT_MAPS_OUT = 3, 8                                    # words per row of tirt_kat_material_maps
HITS_MAX = 64                                                       # TIRT_HITS_MAX: the largest k of tirt_query_hits
NEAREST_MAX = 64                                                    # TIRT_NEAREST_MAX: the largest k of tirt_query_nearest
KAT_LIST_WALK_OUT = 9                                               # words per output row of tirt_kat_primary_list_walk
KAT_STEP_IN, KAT_STEP_OUT = 23, 28                                 # words per row of tirt_kat_shade_step
KAT_SPEC_STEP_IN, KAT_SPEC_STEP_OUT = 23, 29                       # words per row of tirt_kat_shade_spec_step
# tirt_bdpt_record_download: one contribution of BDPT -- frame, source pixel p, target pixel q, strategy (e, l), the three values added
BD_RECORD = np.dtype([("frame", np.int32), ("p", np.int32), ("q", np.int32), ("e", np.int32), ("l", np.int32), ("r", np.float32, (3,))])
# tirt_bdpt_vertices_download: one sub-path vertex (csrc/tirt_bdpt.hip, bvert: five 16-byte quads) and what it returns per item
BD_VERTEX = np.dtype([("pos", np.float32, (3,)), ("prim", np.int32), ("snormal", np.float32, (3,)), ("mat", np.int32), ("normal", np.float32, (3,)), ("fpdf", np.float32),
                      ("beta", np.float32, (3,)), ("rpdf", np.float32), ("wo", np.float32, (3,)), ("type", np.int16), ("delta", np.int16)])
BD_ITEM_ROW = np.dtype([("frame", np.int32), ("pixel", np.int32), ("eye_depth", np.int32), ("tail", np.int32), ("light_depth", np.int32)])
assert BD_RECORD.itemsize == 32 and BD_VERTEX.itemsize == 80

# context options that select code rather than tune it: name -> (default, meaning).  (The tuning options are listed in include/tirt.h.)
OPTIONS = {
    "shade_specialize": (1, "1: the narrowest instantiation of k_shade / k_shade_spec that covers the scene's feature word; 0: the generic kernel"),
}

# name -> (restype, argtypes).  tests/test_abi.py checks every name against include/tirt.h.
_vp = C.c_void_p
SIGNATURES = {
    "tirt_last_error": (C.c_char_p, []),
    "tirt_version": (C.c_int, []),
    "tirt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "tirt_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "tirt_destroy": (None, [_vp]),
    "tirt_sync": (C.c_int, [_vp]),
    "tirt_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "tirt_scene_upload": (C.c_int, [_vp, _f32p, C.c_int, _i32p, C.c_int, _f32p, C.c_int,
                                    _f32p, C.c_int, _i32p, C.c_int, C.c_int, _f32p, _f32p]),
    "tirt_material_upload": (C.c_int, [_vp, _f32p, C.c_int]),
    "tirt_env_upload": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, C.c_float]),
    "tirt_texture_upload": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "tirt_kat_texture": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_kat_material_maps": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_texture_cutout": (C.c_int, [_vp, _vp, C.c_int]),
    "tirt_kat_texture_alpha": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_shade_features": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "tirt_shade_instantiation": (C.c_int, [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "tirt_shade_features_host": (C.c_int, [_f32p, C.c_int, _i32p, C.c_int, _f32p, C.c_int, _i32p, C.c_int, _vp, C.c_int, C.c_int, C.c_float,
                                           C.POINTER(C.c_uint32)]),
    "tirt_shade_features_host_env": (C.c_int, [_f32p, C.c_int, _i32p, C.c_int, _f32p, C.c_int, _i32p, C.c_int, _vp, C.c_int, C.c_int, C.c_float,
                                               C.c_int, C.POINTER(C.c_uint32)]),
    "tirt_env_sampling": (C.c_int, [_vp, C.c_int, C.c_float]),
    "tirt_light_sampling": (C.c_int, [_vp, C.c_int, C.c_float]),
    "tirt_light_table_download": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "tirt_kat_light_pick": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_shade_features_host_lights": (C.c_int, [_f32p, C.c_int, _i32p, C.c_int, _f32p, C.c_int, _i32p, C.c_int, _vp, C.c_int, C.c_int, C.c_float,
                                                  C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "tirt_env_table_download": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "tirt_kat_env_sample": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_kat_env_pdf": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_env_upload_hdr": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_float]),
    "tirt_env_format": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "tirt_kat_env_lookup": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_shade_features_host_env_hdr": (C.c_int, [_f32p, C.c_int, _i32p, C.c_int, _f32p, C.c_int, _i32p, C.c_int, _vp, C.c_int, C.c_int, C.c_float,
                                                   C.c_int, C.c_int, C.POINTER(C.c_uint32)]),
    "tirt_lbvh_build": (C.c_int, [_vp]),
    "tirt_lbvh_download": (C.c_int, [_vp, _vp, _vp, _vp]),
    "tirt_traversal_tree_download": (C.c_int, [_vp, _vp]),
    "tirt_wide_tree_download": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_morton_download": (C.c_int, [_vp, _i32p]),
    "tirt_process_normal": (C.c_int, [_vp, _i32p]),
    "tirt_vertex_download": (C.c_int, [_vp, _f32p]),
    "tirt_vertex_update": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "tirt_vertex_update_device": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "tirt_scene_box": (C.c_int, [_vp, _f32p, _f32p]),
    "tirt_total_area": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "tirt_camera_set": (C.c_int, [_vp, _f32p, _f32p, _f32p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "tirt_film_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "tirt_film_clear": (C.c_int, [_vp]),
    "tirt_pt_rgb_render": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int]),
    "tirt_bdpt_rgb_render": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_uint32]),
    "tirt_bdpt_spec_render": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_uint32]),
    "tirt_bdpt_record_enable": (C.c_int, [_vp, C.c_long]),
    "tirt_bdpt_record_download": (C.c_int, [_vp, _vp, C.c_long, C.POINTER(C.c_long)]),
    "tirt_bdpt_vertices_download": (C.c_int, [_vp, C.POINTER(C.c_int32), _vp, C.c_long, C.POINTER(C.c_long)]),
    "tirt_debug_render": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int]),
    "tirt_tone_map": (C.c_int, [_vp, C.c_float]),
    "tirt_film_download": (C.c_int, [_vp, _vp, _vp]),
    "tirt_film_export_device": (C.c_int, [_vp, _vp]),
    "tirt_film_import_device": (C.c_int, [_vp, _vp]),
    "tirt_aov_enable": (C.c_int, [_vp, C.c_int]),
    "tirt_aov_download": (C.c_int, [_vp, _vp]),
    "tirt_aov_export_device": (C.c_int, [_vp, _vp]),
    "tirt_trace_closest": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _vp]),
    "tirt_trace_shadow": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _i32p, _vp]),
    "tirt_query_closest": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "tirt_query_occluded": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp]),
    "tirt_query_hits": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "tirt_trace_hits": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_hit_list": (C.c_int, [_f32p, C.c_int, C.c_int, C.c_float, _vp, _i32p]),
    "tirt_query_closest_point": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64,
                                           _vp, C.c_int64, _vp, _vp]),
    "tirt_closest_point": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_closest_point": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, _f32p]),
    "tirt_query_nearest": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64,
                                     _vp, C.c_int64, _vp, _vp, _vp]),
    "tirt_nearest": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_nearest_list": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_float, _vp, _vp, _i32p]),
    "tirt_query_mesh_distance": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int64,
                                           _vp, _vp]),
    "tirt_mesh_distance": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_tri_tri": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, _f32p]),
    "tirt_kat_tri_tri_host": (C.c_int, [_f32p, C.c_int, C.c_int, _f32p]),
    "tirt_kat_beam_triangle_host": (C.c_int, [_f32p, C.c_int, C.c_int, _i32p]),
    "tirt_query_sweep": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp,
                                   _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp]),
    "tirt_sweep": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_float, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_sweep": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, _f32p]),
    "tirt_kat_sweep_host": (C.c_int, [_f32p, C.c_int, C.c_int, _f32p]),
    "tirt_query_point_pairs": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                         C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "tirt_point_pairs": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_pairs_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, _vp, _vp, _vp]),
    "tirt_query_mesh_pairs": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                        _vp, C.c_int64, _vp, _vp]),
    "tirt_mesh_pairs": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_query_signed_distance": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int64,
                                             _vp, C.c_int64, _vp, _vp, _vp]),
    "tirt_signed_distance": (C.c_int, [_vp, _f32p, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tirt_signed_distance_prepare": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "tirt_signed_distance_table_download": (C.c_int, [_vp, _f32p]),
    "tirt_kat_signed_distance": (C.c_int, [_vp, _f32p, C.c_int, _f32p]),
    "tirt_query_winding_number": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_float, C.c_int, C.c_int, _vp, _vp, _vp]),
    "tirt_winding_number": (C.c_int, [_vp, _f32p, C.c_int, C.c_float, C.c_int, C.c_int, _vp, _vp]),
    "tirt_winding_prepare": (C.c_int, [_vp]),
    "tirt_winding_table_download": (C.c_int, [_vp, _vp, _vp, _vp]),
    "tirt_kat_winding": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, _vp]),
    "tirt_kat_winding_host": (C.c_int, [_f32p, C.c_int, C.c_int, _vp]),
    "tirt_comm_init": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "tirt_film_reduce": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int]),
    "tirt_comm_destroy": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "tirt_bvh_info": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "tirt_micro_gather_rate": (C.c_int, [_vp, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
    "tirt_trace_timeline": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "tirt_primary_beam_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "tirt_primary_beam_lists_download": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "tirt_kat_primary_list_walk": (C.c_int, [_vp, C.c_int, _i32p, _f32p, _f32p, _f32p, C.c_int]),
    "tirt_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "tirt_stats_reset": (C.c_int, [_vp]),
    "tirt_kat_math": (C.c_int, [_vp, C.c_int, _f32p, _f32p, _f32p, C.c_int]),
    "tirt_kat_brdf": (C.c_int, [_vp, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_kat_spec": (C.c_int, [_vp, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_shade_table_download": (C.c_int, [_vp, C.c_int, _f32p, C.c_uint64]),
    "tirt_kat_shade_tables": (C.c_int, [_vp, C.c_int, _vp, _f32p, C.c_int]),
    "tirt_kat_shade_step": (C.c_int, [_vp, C.c_uint32, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_kat_shade_spec_step": (C.c_int, [_vp, C.c_uint32, _f32p, C.c_int, _f32p, C.c_int, C.c_int]),
    "tirt_obj_load": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "tirt_obj_free": (None, [_vp]),
    "tirt_obj_material_count": (C.c_int, [_vp]),
    "tirt_obj_material_info": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "tirt_obj_material_texture": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int]),
    "tirt_obj_material_map": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "tirt_obj_material_opacity": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int]),
    "tirt_obj_material_vertices": (C.c_int, [_vp, C.c_int, np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"), C.c_longlong]),
}

class SpectralTables(C.Structure):
    """tirt_spectral_t (include/tirt.h)"""
    _fields_ = [("sensor", C.c_void_p), ("n_sensor", C.c_int), ("s_min", C.c_float), ("s_max", C.c_float), ("s_range", C.c_float),
                ("spd", C.c_void_p), ("spd_n", C.c_int * 4), ("spd_min", C.c_float * 4), ("spd_max", C.c_float * 4), ("spd_range", C.c_float * 4),
                ("tbl_scale", C.c_void_p), ("tbl_data", C.c_void_p), ("tbl_res", C.c_int),
                ("sky_cfg", C.c_void_p), ("sky_rad", C.c_void_p), ("sun_dir", C.c_float * 3)]


SIGNATURES.update({
    "tirt_spec_table_build": (C.c_int, [_vp, C.c_int, _f32p, _f32p, C.c_int, _f32p, _f32p]),
    "tirt_spectral_upload": (C.c_int, [_vp, C.POINTER(SpectralTables)]),
    "tirt_pt_spec_render": (C.c_int, [_vp, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int]),
})

class DenoiseParams(C.Structure):
    """tirt_denoise_t (include/tirt.h)"""
    _fields_ = [("levels", C.c_int), ("sigma_c", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float)]


DENOISE_DEFAULTS = {"levels": 5, "sigma_c": 1.0, "sigma_n": 0.3, "sigma_z": 0.1}      # what a NULL tirt_denoise_t means

SIGNATURES.update({
    "tirt_denoise": (C.c_int, [_vp, C.POINTER(DenoiseParams)]),
    "tirt_denoise_download": (C.c_int, [_vp, _vp]),
    "tirt_denoise_export_device": (C.c_int, [_vp, _vp]),
    "tirt_denoise_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(DenoiseParams), _vp]),
})

DENOISE_VAR_DEFAULTS = {"levels": 5, "sigma_c": 3.0, "sigma_n": 0.3, "sigma_z": 0.1}      # what a NULL tirt_denoise_var_t means (TIRT_DENOISE_VAR_SIGMA_C)

SIGNATURES.update({
    "tirt_moments_enable": (C.c_int, [_vp, C.c_int]),
    "tirt_moments_download": (C.c_int, [_vp, _vp]),
    "tirt_moments_export_device": (C.c_int, [_vp, _vp]),
    "tirt_moments_converged": (C.c_int, [_vp, C.c_float, C.POINTER(C.c_uint64)]),
    "tirt_denoise_var": (C.c_int, [_vp, C.POINTER(DenoiseParams)]),      # tirt_denoise_var_t has tirt_denoise_t's fields
    "tirt_denoise_var_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(DenoiseParams), _vp]),
})



class AdaptiveParams(C.Structure):
    """tirt_adaptive_t (include/tirt.h)"""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("pass_frames", C.c_int32)]


class AdaptiveResult(C.Structure):
    """tirt_adaptive_result_t (include/tirt.h)"""
    _fields_ = [("passes", C.c_int64), ("pixel_samples", C.c_int64), ("pixels_at_max", C.c_int64), ("frames", C.c_int64)]


SIGNATURES.update({
    "tirt_pixel_set_upload": (C.c_int, [_vp, _vp, C.c_int64]),
    "tirt_pixel_set_from_moments": (C.c_int, [_vp, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "tirt_pixel_set_clear": (C.c_int, [_vp]),
    "tirt_pixel_set_download": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    "tirt_pt_rgb_render_adaptive": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveResult)]),
})

class TemporalParams(C.Structure):
    """tirt_temporal_t (include/tirt.h)"""
    _fields_ = [("max_history", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float)]


class TemporalCamera(C.Structure):
    """tirt_temporal_camera_t (include/tirt.h): what tirt_camera_set takes"""
    _fields_ = [("view", C.c_float * 16), ("view_inv", C.c_float * 16), ("eye", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


TEMPORAL_DEFAULTS = {"max_history": 32.0, "sigma_n": 0.3, "sigma_z": 0.1}      # what a NULL tirt_temporal_t means (TIRT_TEMPORAL_MAX_HISTORY)

SIGNATURES.update({
    "tirt_temporal_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(TemporalCamera), C.POINTER(TemporalCamera), _vp, _vp, C.c_int, C.c_int,
                                       C.POINTER(TemporalParams), _vp]),
    "tirt_temporal_enable": (C.c_int, [_vp, C.c_int]),
    "tirt_temporal_accumulate": (C.c_int, [_vp, C.POINTER(TemporalParams)]),
    "tirt_temporal_reset": (C.c_int, [_vp]),
    "tirt_temporal_download": (C.c_int, [_vp, _vp, _vp]),
    "tirt_temporal_export_device": (C.c_int, [_vp, _vp, _vp]),
    "tirt_temporal_denoise_var": (C.c_int, [_vp, C.POINTER(DenoiseParams)]),
})


SIGNATURES.update({
    "tirt_motion_enable": (C.c_int, [_vp, C.c_int]),
    "tirt_motion_download": (C.c_int, [_vp, _vp]),
    "tirt_motion_export_device": (C.c_int, [_vp, _vp]),
    "tirt_motion_temporal_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(TemporalCamera), C.POINTER(TemporalCamera), _vp, _vp, C.c_int,
                                              C.c_int, C.POINTER(TemporalParams), _vp, _vp]),
})


def temporal_camera(cam):
    """a TemporalCamera from a Camera (or anything with view_np, view_inv_np, eye_np, fx, fy, cx, cy) or from the tuple Camera pushes to tirt_camera_set:
    (view, view_inv, eye, fx, fy, cx, cy)"""
    if isinstance(cam, TemporalCamera):
        return cam
    if hasattr(cam, "view_np"):
        cam = (cam.view_np[0], cam.view_inv_np[0], cam.eye_np[0], cam.fx, cam.fy, cam.cx, cam.cy)
    view, view_inv, eye, fx, fy, cx, cy = cam
    view, view_inv, eye = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (view, view_inv, eye))
    if view.size != 16 or view_inv.size != 16 or eye.size != 3:
        raise ValueError("a camera is (view[4, 4], view_inv[4, 4], eye[3], fx, fy, cx, cy)")
    out = TemporalCamera()
    out.view[:] = view.tolist(); out.view_inv[:] = view_inv.tolist(); out.eye[:] = eye.tolist()
    out.fx, out.fy, out.cx, out.cy = float(fx), float(fy), float(cx), float(cy)
    return out


_lib = None


def _prefer_torch_hip_runtime():
    """PyTorch-ROCm ships its own HIP runtime under the SONAME of the system one (libamdhip64.so.7); whichever is loaded first serves the
    whole process, and torch.cuda does not come up on the system one ("No HIP GPUs are available" after this library initialised HIP).
    So torch's copy is loaded first -- without importing torch -- when there is one: libtirt.so runs on it as it does when the
    application imported torch before this package (bench.py, the multi-GPU path).  TIRT_SYSTEM_HIP=1 keeps the system runtime."""
    if os.environ.get("TIRT_SYSTEM_HIP", "0") not in ("", "0") or os.environ.get("TIRT_NO_ENV_TUNING", "0") not in ("", "0"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass                                   # no torch, or a torch without a bundled runtime: the system one


def _check_one_hip_runtime():
    """libtirt.so needs `libamdhip64.so.7` (DT_NEEDED, by SONAME).  The preload above only satisfies that when torch's bundled runtime carries
    the same SONAME; a wheel with another (or a hashed) name leaves the loader to pull in the system runtime as well -- two HIP runtimes in one
    process, each with its own devices, streams and allocations.  Say so instead of failing later in some unrelated call."""
    try:
        with open("/proc/self/maps") as f:
            libs = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return
    if len({os.path.realpath(p) for p in libs}) > 1:
        msg = ("two HIP runtimes are mapped into this process (%s): libtirt.so and PyTorch will not see each other's device memory; "
               "set TIRT_SYSTEM_HIP=1 (and import torch after this package), or make the SONAMEs agree" % ", ".join(libs))
        if os.environ.get("TIRT_ALLOW_TWO_HIP_RUNTIMES", "0") in ("", "0"):       # loud by default (round-4 review); a process that never hands device pointers across may opt out
            raise TirtError(msg + " -- or TIRT_ALLOW_TWO_HIP_RUNTIMES=1 if the two never exchange device pointers")
        import warnings
        warnings.warn(msg, RuntimeWarning)


def lib():
    """Load libtirt.so once.  Raises TirtError (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TirtError(
                "HIP extension %s is missing -- build it with `python -c 'import "
                "__graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback." % LIB_PATH)
        _prefer_torch_hip_runtime()
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise TirtError("cannot load %s: %s" % (LIB_PATH, exc))
        _check_one_hip_runtime()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code):
    if code != 0:
        msg = lib().tirt_last_error()
        raise TirtError("libtirt error %d: %s" % (code, msg.decode() if msg else "?"))


def _ptr(arr):
    return None if arr is None else arr.ctypes.data_as(C.c_void_p)


def _bound(value, n):
    """a per-query bound of the host routes (max_distance, tmax, radius): None stays None, a float or (n,) array becomes contiguous (n,) float32"""
    return None if value is None else np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float32), (n,)))


def _kat_rows(symbol, handle, head, rows, out_stride, words=False, in_stride=None):
    """One known-answer entry over a table of rows: symbol(handle, *head, rows, in_stride, out, out_stride, n) -> the zero-initialised (n, out_stride) float32.
    words: the rows are 32-bit words taken as their bits (integers ride in them); otherwise they are converted to float32."""
    rows = np.ascontiguousarray(rows).view(np.float32) if words else np.ascontiguousarray(rows, np.float32)
    n, stride = rows.shape
    out = np.zeros((n, max(int(out_stride), 1)), np.float32)
    check(getattr(lib(), symbol)(handle, *head, rows.reshape(-1), int(stride if in_stride is None else in_stride), out.reshape(-1), int(out_stride), n))
    return out


class Context:
    """RAII wrapper around tirt_ctx*."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        check(lib().tirt_create(int(device_id), C.byref(self._h)))
        self.device_id = int(device_id)
        self._bdpt_record_cap = -1                 # what bdpt_record_enable asked for (bdpt_record_download returns no more than the device kept)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().tirt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h.value:
            raise TirtError("context is closed")
        return self._h

    # thin typed wrappers ---------------------------------------------------------------
    def sync(self):
        check(lib().tirt_sync(self.handle))

    def set_option(self, name, value):
        check(lib().tirt_set_option(self.handle, name.encode(), float(value)))

    def scene_upload(self, vertex, primitive, material, shape, light, light_count, bmin, bmax):
        vertex = np.ascontiguousarray(vertex, np.float32)
        primitive = np.ascontiguousarray(primitive, np.int32)
        material = np.ascontiguousarray(material, np.float32)
        shape = np.ascontiguousarray(shape, np.float32)
        light = np.ascontiguousarray(light, np.int32)
        check(lib().tirt_scene_upload(
            self.handle, vertex.reshape(-1), vertex.shape[0], primitive.reshape(-1), primitive.shape[0],
            material.reshape(-1), material.shape[0], shape.reshape(-1), shape.shape[0],
            light.reshape(-1), light.shape[0], int(light_count),
            np.ascontiguousarray(bmin, np.float32).reshape(-1), np.ascontiguousarray(bmax, np.float32).reshape(-1)))

    def material_upload(self, material):
        material = np.ascontiguousarray(material, np.float32)
        check(lib().tirt_material_upload(self.handle, material.reshape(-1), material.shape[0]))

    def env_upload(self, packed, power):
        packed = np.ascontiguousarray(packed, np.int32)
        check(lib().tirt_env_upload(self.handle, packed.reshape(-1), packed.shape[0], packed.shape[1], float(power)))

    def env_upload_hdr(self, packed, power):
        """include/tirt.h, tirt_env_upload_hdr: packed [w, h] int32 RGBE8 texels (Texture.np_img of load_hdr / load_array_float)"""
        env_upload_hdr(self.handle, packed, power)

    def env_format(self):
        """include/tirt.h, tirt_env_format: (format 0 8-bit / 1 RGBE8, E_max of the sampling table's scale)"""
        out = (C.c_int32 * 2)()
        check(lib().tirt_env_format(self.handle, out))
        return int(out[0]), int(out[1])

    def kat_env_lookup(self, rows, out_stride=KAT_ENV_LOOKUP_OUT):
        """include/tirt.h, tirt_kat_env_lookup: rows (n, >= 2) float32 (tx, ty) -> (n, out_stride) float32: the environment's linear colour before env_power"""
        return _kat_rows("tirt_kat_env_lookup", self.handle, (), rows, out_stride)

    def texture_upload(self, textures):
        """include/tirt.h, tirt_texture_upload: `textures` is a sequence of (packed [w, h] int32 as Texture.np_img, wrap 0 clamp / 1 repeat); empty: remove all"""
        texture_upload(self.handle, textures)

    def kat_texture(self, rows, out_stride=6):
        """include/tirt.h, tirt_kat_texture: rows (n, >= 3) of 32-bit words (texture number as its bits, u, v) -> (n, out_stride) float32: c3, srgb_to_lrgb(c)3"""
        return _kat_rows("tirt_kat_texture", self.handle, (), rows, out_stride, words=True)

    def texture_cutout(self, flags):
        """include/tirt.h, tirt_texture_cutout: one 0 / 1 per uploaded texture -- is its top byte (255 - alpha) a cut-out mask"""
        texture_cutout(self.handle, flags)

    def kat_texture_alpha(self, rows, out_stride=KAT_ALPHA_OUT):
        """include/tirt.h, tirt_kat_texture_alpha: rows (n, >= 3) of 32-bit words (texture number as its bits, u, v) -> (n, out_stride) float32: alpha, decision"""
        return _kat_rows("tirt_kat_texture_alpha", self.handle, (), rows, out_stride, words=True)

    def kat_material_maps(self, rows, out_stride=KAT_MAPS_OUT):
        """include/tirt.h, tirt_kat_material_maps: rows (n, >= 3) of 32-bit words (primitive as its bits, hit u, hit v) -> (n, out_stride) float32: uv2, rough, metal, N'3, 0"""
        return _kat_rows("tirt_kat_material_maps", self.handle, (), rows, out_stride, words=True)

    def env_sampling(self, on, share=0.5):
        """include/tirt.h, tirt_env_sampling: importance-sample the environment in PT_RGB (NEE + MIS); share of the light samples it gets beside emitters"""
        env_sampling(self.handle, on, share)

    def light_sampling(self, power, uniform_share=0.0):
        """include/tirt.h, tirt_light_sampling: choose PT_RGB's emitter samples by power (True) or uniformly over the light list; the share that stays uniform"""
        light_sampling(self.handle, 1 if power else 0, uniform_share)

    def light_table_download(self):
        """include/tirt.h, tirt_light_table_download: None without a table, else {"count", "e_max", "active", "q" [N] uint32, "prefix" [N] uint64, "P" [N] float32}"""
        info = (C.c_int32 * 4)()
        check(lib().tirt_light_table_download(self.handle, None, None, None, info))
        if not info[3]:
            return None
        n = int(info[0])
        q, prefix, P = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.float32)
        check(lib().tirt_light_table_download(self.handle, _ptr(q), _ptr(prefix), _ptr(P), info))
        return {"count": n, "e_max": int(info[1]), "active": bool(info[2]), "q": q, "prefix": prefix, "P": P}

    def kat_light_pick(self, r):
        """include/tirt.h, tirt_kat_light_pick: r (n,) float32 in [0, 1] -> (index (n,) int32, P (n,) float32)"""
        r = np.ascontiguousarray(r, np.float32).reshape(-1)
        out = np.zeros((r.shape[0], KAT_LIGHT_PICK_OUT), np.float32)
        check(lib().tirt_kat_light_pick(self.handle, r, 1, out.reshape(-1), KAT_LIGHT_PICK_OUT, r.shape[0]))
        return out[:, 0].copy().view(np.int32), out[:, 1].copy()

    def env_table_download(self):
        """include/tirt.h, tirt_env_table_download: None without a table, else {"w", "h", "active", "q" [h, w] uint32, "row_sums" [h, w] uint64, "marginal" [h] uint64}"""
        info = (C.c_int32 * 4)()
        check(lib().tirt_env_table_download(self.handle, None, None, None, info))
        if not info[2]:
            return None
        w, h = int(info[0]), int(info[1])
        q, rows, marg = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint64), np.zeros(h, np.uint64)
        check(lib().tirt_env_table_download(self.handle, _ptr(q), _ptr(rows), _ptr(marg), info))
        return {"w": w, "h": h, "active": bool(info[3]), "q": q, "row_sums": rows, "marginal": marg}

    def kat_env_sample(self, rows, out_stride=KAT_ENV_SAMPLE_OUT):
        """include/tirt.h, tirt_kat_env_sample: rows (n, >= 2) float32 (ra, rb) -> (n, out_stride) float32: i, j (bits), tx, ty, d3, pdf, lookup cell i, j (bits)"""
        return _kat_rows("tirt_kat_env_sample", self.handle, (), rows, out_stride)

    def kat_env_pdf(self, rows, out_stride=KAT_ENV_PDF_OUT):
        """include/tirt.h, tirt_kat_env_pdf: rows (n, >= 3) float32 directions -> (n, out_stride) float32: i, j (bits), tx, ty, pdf"""
        return _kat_rows("tirt_kat_env_pdf", self.handle, (), rows, out_stride)

    def shade_features(self):
        """(feature word, shade_specialize option) of the context: include/tirt.h, tirt_shade_features"""
        out = (C.c_uint32 * 2)()
        check(lib().tirt_shade_features(self.handle, out))
        return int(out[0]), int(out[1])

    def lbvh_build(self):
        check(lib().tirt_lbvh_build(self.handle))

    def lbvh_download(self, n, want_morton=True, want_bvh=True, want_compact=True):
        N = 2 * n - 1
        morton = np.zeros((n, 2), np.int32) if want_morton else None
        bvh = np.zeros((N, 11), np.float32) if want_bvh else None
        compact = np.zeros((N, 9), np.float32) if want_compact else None
        check(lib().tirt_lbvh_download(self.handle, _ptr(morton), _ptr(bvh), _ptr(compact)))
        return morton, bvh, compact

    def traversal_tree_download(self, n):
        """rows [(2n-1), 9] of the tree the ordered traversal walks (tirt.h)"""
        rows = np.zeros((2 * n - 1, 9), np.float32)
        check(lib().tirt_traversal_tree_download(self.handle, _ptr(rows)))
        return rows

    def wide_tree_download(self, n):
        """What the ordered and the exhaustive traversal walk, as lbvh_build left it (tirt.h, tirt_wide_tree_download): a dict with cnode
        uint32 [wide_nodes + n_far_nodes, 16], tri float32 [n, 12], wnode float32 [2n-1, 16] (rows of leaves are not written), prim_slot
        int32 [n], the grid (grid_min, grid_cell, grid_inv_cell, grid_inv_extent, root_min, root_max: float32 [3]), pad (np.float32)
        and the integers wide_nodes, n_far_nodes, root_code, far_qcode, built_sah, shapes_boxed."""
        grid = np.zeros(19, np.float32); info = np.zeros(6, np.int32)
        check(lib().tirt_wide_tree_download(self.handle, None, None, None, None, _ptr(grid), _ptr(info)))
        out = {"cnode": np.zeros((int(info[0]) + int(info[1]), 16), np.uint32), "tri": np.zeros((n, 12), np.float32),
               "wnode": np.zeros((2 * n - 1, 16), np.float32), "prim_slot": np.zeros(n, np.int32)}
        check(lib().tirt_wide_tree_download(self.handle, _ptr(out["cnode"]), _ptr(out["tri"]), _ptr(out["wnode"]), _ptr(out["prim_slot"]),
                                            _ptr(grid), _ptr(info)))
        for k, name in enumerate(("grid_min", "grid_cell", "grid_inv_cell", "grid_inv_extent", "root_min", "root_max")):
            out[name] = grid[3 * k:3 * k + 3].copy()
        out["pad"] = np.float32(grid[18])
        for k, name in enumerate(("wide_nodes", "n_far_nodes", "root_code", "far_qcode", "built_sah", "shapes_boxed")):
            out[name] = int(info[k])
        return out

    def morton_download(self, n):
        out = np.zeros((n, 2), np.int32)
        check(lib().tirt_morton_download(self.handle, out.reshape(-1)))
        return out

    def process_normal(self, vertex_index):
        check(lib().tirt_process_normal(self.handle, np.ascontiguousarray(vertex_index, np.int32)))

    def vertex_download(self, nv):
        out = np.zeros((nv, 9), np.float32)
        check(lib().tirt_vertex_download(self.handle, out.reshape(-1)))
        return out

    def vertex_update(self, first, count, pos, pos_stride=3, nrm=0, nrm_stride=3, device=False, stream=0):
        """tirt_vertex_update (device=False: `pos` / `nrm` are integer HOST addresses) or tirt_vertex_update_device (integer device
        addresses, `stream` a hipStream_t handle, 0 = the null stream).  nrm = 0: face normals.  Strides in floats.  The LBVH counts as
        not built afterwards: lbvh_build() next (include/tirt.h)."""
        if device:
            check(lib().tirt_vertex_update_device(self.handle, int(first), int(count), _vp(int(pos) or None), int(pos_stride),
                                                  _vp(int(nrm) or None), int(nrm_stride), _vp(int(stream) or None)))
        else:
            check(lib().tirt_vertex_update(self.handle, int(first), int(count), _vp(int(pos) or None), int(pos_stride),
                                           _vp(int(nrm) or None), int(nrm_stride)))

    def scene_box(self):
        """(bmin[3], bmax[3]) float32: the scene box as the context holds it"""
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(lib().tirt_scene_box(self.handle, lo, hi))
        return lo, hi

    def total_area(self):
        v = C.c_float(0.0)
        check(lib().tirt_total_area(self.handle, C.byref(v)))
        return float(v.value)

    def camera_set(self, view, view_inv, eye, fx, fy, cx, cy):
        check(lib().tirt_camera_set(
            self.handle, np.ascontiguousarray(view, np.float32).reshape(-1),
            np.ascontiguousarray(view_inv, np.float32).reshape(-1),
            np.ascontiguousarray(eye, np.float32).reshape(-1), float(fx), float(fy), float(cx), float(cy)))

    def film_create(self, W, H, tile_rank=0, tile_count=1, tile_size=4096):
        check(lib().tirt_film_create(self.handle, int(W), int(H), int(tile_rank), int(tile_count), int(tile_size)))

    def film_clear(self):
        check(lib().tirt_film_clear(self.handle))

    def pt_rgb_render(self, frame_begin, frame_count, seed, max_depth=15, stack_size=64, flags=0):
        check(lib().tirt_pt_rgb_render(self.handle, int(frame_begin), int(frame_count), int(seed),
                                       int(max_depth), int(stack_size), int(flags)))

    def bdpt_rgb_render(self, frame_begin, frame_count, seed):
        check(lib().tirt_bdpt_rgb_render(self.handle, int(frame_begin), int(frame_count), int(seed)))

    def bdpt_spec_render(self, frame_begin, frame_count, seed):
        check(lib().tirt_bdpt_spec_render(self.handle, int(frame_begin), int(frame_count), int(seed)))

    def bdpt_record_enable(self, capacity):
        """capacity >= 0: the BDPT renders from now on also write their contributions (BD_RECORD) and the count restarts; < 0: off"""
        check(lib().tirt_bdpt_record_enable(self.handle, int(capacity)))
        self._bdpt_record_cap = int(capacity)

    def bdpt_record_download(self, capacity=None, out=None):
        """(records, needed): what the BDPT renders since bdpt_record_enable wrote, in no defined order, and how many records they needed -- more than
        len(records) when the enabled capacity (or `capacity` / `out` here) was too small.  capacity None: as many as were needed (or as `out` holds)."""
        need = C.c_long(0)
        if out is None:
            if capacity is None:
                check(lib().tirt_bdpt_record_download(self.handle, None, 0, C.byref(need)))
                capacity = need.value
            out = np.zeros(int(capacity), BD_RECORD)
        else:
            assert out.dtype == BD_RECORD and out.flags["C_CONTIGUOUS"]
            capacity = len(out) if capacity is None else min(int(capacity), len(out))
        check(lib().tirt_bdpt_record_download(self.handle, out.ctypes.data_as(_vp), int(capacity), C.byref(need)))
        return out[:max(0, min(int(capacity), need.value, self._bdpt_record_cap))], need.value          # (what was kept: not more than the enabled capacity)

    def bdpt_vertices_download(self):
        """(rows, vertices) of the last BDPT call, which must have run as one batch: rows[n] (frame, pixel, eye_depth, tail, light_depth) and
        vertices[n, 13] of BD_VERTEX (eye slots 0..6, light slots 7..12) as the kernels left them"""
        n = C.c_long(0)
        check(lib().tirt_bdpt_vertices_download(self.handle, None, None, 0, C.byref(n)))
        raw = np.zeros((n.value, 4), np.int32)
        verts = np.zeros((n.value, 13), BD_VERTEX)
        check(lib().tirt_bdpt_vertices_download(self.handle, raw.ctypes.data_as(C.POINTER(C.c_int32)), verts.ctypes.data_as(_vp), n.value, C.byref(n)))
        rows = np.zeros(n.value, BD_ITEM_ROW)
        rows["frame"], rows["pixel"], rows["light_depth"] = raw[:, 0], raw[:, 1], raw[:, 3]
        rows["eye_depth"], rows["tail"] = raw[:, 2] & 0xffff, raw[:, 2] >> 16
        return rows, verts

    def pt_spec_render(self, frame_begin, frame_count, seed, max_depth=10, stack_size=64, flags=0):
        check(lib().tirt_pt_spec_render(self.handle, int(frame_begin), int(frame_count), int(seed),
                                        int(max_depth), int(stack_size), int(flags)))

    def spec_table_build(self, res, cie_xyz, d65):
        cie_xyz = np.ascontiguousarray(cie_xyz, np.float32).reshape(-1)
        d65 = np.ascontiguousarray(d65, np.float32)
        scale = np.zeros(res, np.float32)
        coeff = np.zeros(9 * res * res * res, np.float32)
        check(lib().tirt_spec_table_build(self.handle, int(res), cie_xyz, d65, int(d65.size), scale, coeff))
        return scale, coeff

    def spectral_upload(self, t):
        """t: the dict of PT_Spec.PathTrace.tables()"""
        keep = [np.ascontiguousarray(t[k], np.float32) for k in ("sensor", "spd", "tbl_scale", "tbl_data", "sky_cfg", "sky_rad")]
        st = SpectralTables()
        st.sensor, st.spd, st.tbl_scale, st.tbl_data, st.sky_cfg, st.sky_rad = [a.ctypes.data for a in keep]
        st.n_sensor = int(t["n_sensor"]); st.s_min = t["s_min"]; st.s_max = t["s_max"]; st.s_range = t["s_range"]
        for k in range(4):
            st.spd_n[k] = int(t["spd_n"][k]); st.spd_min[k] = t["spd_min"][k]; st.spd_max[k] = t["spd_max"][k]; st.spd_range[k] = t["spd_range"][k]
        st.tbl_res = int(t["tbl_res"])
        for k in range(3):
            st.sun_dir[k] = t["sun_dir"][k]
        check(lib().tirt_spectral_upload(self.handle, C.byref(st)))

    def debug_render(self, frame, seed, mode, stack_size=64, flags=0):
        check(lib().tirt_debug_render(self.handle, int(frame), int(seed), int(mode), int(stack_size), int(flags)))

    def tone_map(self, exposure):
        check(lib().tirt_tone_map(self.handle, float(exposure)))

    def film_download(self, W, H, want_hdr=True, want_rgb=False):
        hdr = np.zeros((W, H, 3), np.float32) if want_hdr else None
        rgb = np.zeros((W, H, 3), np.float32) if want_rgb else None
        check(lib().tirt_film_download(self.handle, _ptr(hdr), _ptr(rgb)))
        return hdr, rgb

    def _record_download(self, symbol, W, H, words):
        """[W, H, words] float32 from one of the tirt_*_download entry points"""
        out = np.zeros((W, H, words), np.float32)
        check(getattr(lib(), symbol)(self.handle, _ptr(out)))
        return out

    def _export(self, symbol, dev_ptr):
        """the tirt_*_export_device / tirt_film_import_device entry points: one device address"""
        check(getattr(lib(), symbol)(self.handle, C.c_void_p(int(dev_ptr))))

    @staticmethod
    def _denoise_params(levels, sigma_c, sigma_n, sigma_z):
        return DenoiseParams(int(levels), float(sigma_c), float(sigma_n), float(sigma_z))

    def _denoise_device(self, symbol, arrays, W, H, levels, sigma_c, sigma_n, sigma_z, stream):
        check(getattr(lib(), symbol)(self.handle, *[_vp(int(a) or None) for a in arrays], int(W), int(H),
                                     C.byref(self._denoise_params(levels, sigma_c, sigma_n, sigma_z)), _vp(int(stream) or None)))

    def film_export_device(self, dev_ptr):
        self._export("tirt_film_export_device", dev_ptr)

    def film_import_device(self, dev_ptr):
        self._export("tirt_film_import_device", dev_ptr)

    def aov_enable(self, on=True):
        """tirt_aov_enable: the feature buffers of the film (include/tirt.h), zeroed; on=False frees them"""
        check(lib().tirt_aov_enable(self.handle, 1 if on else 0))

    def aov_download(self, W, H):
        """[W, H, AOV_WORDS] float32: albedo3, normal3, depth, alpha per pixel"""
        return self._record_download("tirt_aov_download", W, H, AOV_WORDS)

    def aov_export_device(self, dev_ptr):
        self._export("tirt_aov_export_device", dev_ptr)

    def moments_enable(self, on=True):
        """tirt_moments_enable: the sample moments of the film (include/tirt.h), zeroed; on=False frees them"""
        check(lib().tirt_moments_enable(self.handle, 1 if on else 0))

    def moments_download(self, W, H):
        """[W, H, MOM_WORDS] float32: n, mean3, M2 3, bad per pixel"""
        return self._record_download("tirt_moments_download", W, H, MOM_WORDS)

    def moments_export_device(self, dev_ptr):
        self._export("tirt_moments_export_device", dev_ptr)

    def moments_converged(self, threshold):
        """tirt_moments_converged: (measured pixels, measured pixels whose standard error exceeds threshold x their mean level, pixels with skipped samples)"""
        out = (C.c_uint64 * 3)()
        check(lib().tirt_moments_converged(self.handle, float(threshold), out))
        return int(out[0]), int(out[1]), int(out[2])

    def pixel_set_upload(self, pixels):
        """tirt_pixel_set_upload: restrict the next pt_rgb_render calls to these linear pixel indices (p = i*H + j) of this context's tiles, strictly
        ascending in the context's local order (include/tirt.h); an empty list installs the empty set"""
        px = np.ascontiguousarray(pixels, np.int32).reshape(-1)
        check(lib().tirt_pixel_set_upload(self.handle, _ptr(px) if px.size else None, px.size))

    def pixel_set_from_moments(self, threshold, min_samples, max_samples):
        """tirt_pixel_set_from_moments: the set of the pixels still noisy by the moment records, made on the device; returns its length"""
        count = C.c_int64(0)
        check(lib().tirt_pixel_set_from_moments(self.handle, float(threshold), int(min_samples), int(max_samples), C.byref(count)))
        return int(count.value)

    def pixel_set_clear(self):
        check(lib().tirt_pixel_set_clear(self.handle))

    def pixel_set_download(self):
        """tirt_pixel_set_download: the installed list as int32 [n], or None when no set is installed"""
        n = C.c_int64(0)
        check(lib().tirt_pixel_set_download(self.handle, None, 0, C.byref(n)))
        if n.value < 0:
            return None
        out = np.zeros(max(int(n.value), 1), np.int32)
        check(lib().tirt_pixel_set_download(self.handle, _ptr(out), out.size, C.byref(n)))
        return out[:int(n.value)].copy()

    def pt_rgb_render_adaptive(self, frame_begin, seed, threshold, max_samples, min_samples=4, pass_frames=4, max_depth=15, stack_size=64, flags=0):
        """tirt_pt_rgb_render_adaptive: pass after pass of pass_frames frames from frame_begin on, each on the pixels the moment records still call
        noisy, until none is left or every pixel has max_samples; returns {passes, pixel_samples, pixels_at_max, frames}"""
        prm = AdaptiveParams(float(threshold), int(min_samples), int(max_samples), int(pass_frames))
        res = AdaptiveResult()
        check(lib().tirt_pt_rgb_render_adaptive(self.handle, int(frame_begin), int(seed), int(max_depth), int(stack_size), int(flags), C.byref(prm), C.byref(res)))
        return {"passes": int(res.passes), "pixel_samples": int(res.pixel_samples), "pixels_at_max": int(res.pixels_at_max), "frames": int(res.frames)}

    def denoise_var(self, levels=5, sigma_c=DENOISE_VAR_DEFAULTS["sigma_c"], sigma_n=0.3, sigma_z=0.1):
        """tirt_denoise_var: the variance-guided a-trous filter over the context's film, feature buffers and sample moments, into the buffer
        denoise_download reads (include/tirt.h); asynchronous"""
        check(lib().tirt_denoise_var(self.handle, C.byref(self._denoise_params(levels, sigma_c, sigma_n, sigma_z))))

    def denoise_var_device(self, hdr, aov, mom, out, W, H, levels=5, sigma_c=DENOISE_VAR_DEFAULTS["sigma_c"], sigma_n=0.3, sigma_z=0.1, stream=0):
        """tirt_denoise_var_device on device memory: as denoise_device, with mom [W, H, 8] the sample moments"""
        self._denoise_device("tirt_denoise_var_device", (hdr, aov, mom, out), W, H, levels, sigma_c, sigma_n, sigma_z, stream)

    def temporal_enable(self, on=True):
        """tirt_temporal_enable: the context's history of accumulated views (include/tirt.h), empty; needs the feature buffers and the sample moments"""
        check(lib().tirt_temporal_enable(self.handle, 1 if on else 0))

    def temporal_accumulate(self, max_history=TEMPORAL_DEFAULTS["max_history"], sigma_n=0.3, sigma_z=0.1):
        """tirt_temporal_accumulate: the history reprojected into the camera set now and merged with the film and its moment records; asynchronous"""
        check(lib().tirt_temporal_accumulate(self.handle, C.byref(TemporalParams(float(max_history), float(sigma_n), float(sigma_z)))))

    def temporal_reset(self):
        check(lib().tirt_temporal_reset(self.handle))

    def temporal_download(self, W, H, want_hdr=True, want_mom=True):
        """(hdr [W, H, 3], moments [W, H, MOM_WORDS]) float32 of the accumulated film; None for what is not wanted"""
        hdr = np.zeros((W, H, 3), np.float32) if want_hdr else None
        mom = np.zeros((W, H, MOM_WORDS), np.float32) if want_mom else None
        check(lib().tirt_temporal_download(self.handle, _ptr(hdr), _ptr(mom)))
        return hdr, mom

    def temporal_export_device(self, hdr_ptr, mom_ptr):
        """tirt_temporal_export_device: integer device addresses, 0 for what is not wanted"""
        check(lib().tirt_temporal_export_device(self.handle, _vp(int(hdr_ptr) or None), _vp(int(mom_ptr) or None)))

    def temporal_denoise_var(self, levels=5, sigma_c=DENOISE_VAR_DEFAULTS["sigma_c"], sigma_n=0.3, sigma_z=0.1):
        """tirt_temporal_denoise_var: tirt_denoise_var's filter over the accumulated film, into the buffer denoise_download reads; asynchronous"""
        check(lib().tirt_temporal_denoise_var(self.handle, C.byref(self._denoise_params(levels, sigma_c, sigma_n, sigma_z))))

    def temporal_device(self, hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cam, cam_prev, hdr_o, mom_o, W, H,
                        max_history=TEMPORAL_DEFAULTS["max_history"], sigma_n=0.3, sigma_z=0.1, stream=0):
        """tirt_temporal_device on device memory: the arrays are integer device addresses, the cameras what temporal_camera takes, `stream` a
        hipStream_t handle (0 = the null stream).  Asynchronous; ti_raytrace_amd.temporal_accumulate is the torch front end."""
        check(lib().tirt_temporal_device(self.handle, *[_vp(int(a) or None) for a in (hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h)],
                                         C.byref(temporal_camera(cam)), C.byref(temporal_camera(cam_prev)), _vp(int(hdr_o) or None), _vp(int(mom_o) or None),
                                         int(W), int(H), C.byref(TemporalParams(float(max_history), float(sigma_n), float(sigma_z))), _vp(int(stream) or None)))

    def motion_enable(self, on=True):
        """tirt_motion_enable: motion records for the temporal accumulation (include/tirt.h): geometry updates then keep the history; needs temporal_enable"""
        check(lib().tirt_motion_enable(self.handle, 1 if on else 0))

    def motion_download(self, W, H):
        """[W, H, MOTION_WORDS] float32: the motion records of the last temporal_accumulate (D3, 1, dN3, 0 per pixel; zeros where nothing moved)"""
        return self._record_download("tirt_motion_download", W, H, MOTION_WORDS)

    def motion_export_device(self, dev_ptr):
        self._export("tirt_motion_export_device", dev_ptr)

    def motion_temporal_device(self, hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h, cam, cam_prev, hdr_o, mom_o, W, H, motion,
                           max_history=TEMPORAL_DEFAULTS["max_history"], sigma_n=0.3, sigma_z=0.1, stream=0):
        """tirt_motion_temporal_device: temporal_device with `motion`, the device address of [W, H, MOTION_WORDS] motion records"""
        check(lib().tirt_motion_temporal_device(self.handle, *[_vp(int(a) or None) for a in (hdr_c, aov_c, mom_c, hdr_h, aov_h, mom_h)],
                                                C.byref(temporal_camera(cam)), C.byref(temporal_camera(cam_prev)), _vp(int(hdr_o) or None), _vp(int(mom_o) or None),
                                                int(W), int(H), C.byref(TemporalParams(float(max_history), float(sigma_n), float(sigma_z))),
                                                _vp(int(motion) or None), _vp(int(stream) or None)))

    def denoise(self, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1):
        """tirt_denoise: the a-trous filter over the context's film and feature buffers into a buffer of its own (include/tirt.h); asynchronous"""
        check(lib().tirt_denoise(self.handle, C.byref(self._denoise_params(levels, sigma_c, sigma_n, sigma_z))))

    def denoise_download(self, W, H):
        """[W, H, 3] float32: the filtered film of the last denoise()"""
        return self._record_download("tirt_denoise_download", W, H, 3)

    def denoise_export_device(self, dev_ptr):
        self._export("tirt_denoise_export_device", dev_ptr)

    def denoise_device(self, hdr, aov, out, W, H, levels=5, sigma_c=1.0, sigma_n=0.3, sigma_z=0.1, stream=0):
        """tirt_denoise_device on device memory: hdr [W, H, 3], aov [W, H, 8], out [W, H, 3] are integer device addresses, `stream` a hipStream_t
        handle (0 = the null stream).  Asynchronous; ti_raytrace_amd.denoise is the torch front end."""
        self._denoise_device("tirt_denoise_device", (hdr, aov, out), W, H, levels, sigma_c, sigma_n, sigma_z, stream)

    def trace_closest(self, rays, stack_size=64, flags=0):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        nr = rays.shape[0]
        out = np.zeros((nr, 13), np.float32)
        prim = np.zeros(nr, np.int32)
        counts = np.zeros((nr, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_trace_closest(self.handle, rays.reshape(-1), nr, int(stack_size), int(flags),
                                       out.reshape(-1), prim, _ptr(counts)))
        return out, prim, counts

    def trace_shadow(self, rays, stack_size=64, flags=0):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        nr = rays.shape[0]
        out = np.zeros(nr, np.float32)
        prim = np.zeros(nr, np.int32)
        counts = np.zeros((nr, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_trace_shadow(self.handle, rays.reshape(-1), nr, int(stack_size), int(flags),
                                      out, prim, _ptr(counts)))
        return out, prim, counts

    def query_closest(self, rays, nr, ray_stride, stack_size=64, flags=0, out_t=0, out_prim=0, out_hit=0, hit_stride=13, counts=0, stream=0):
        """tirt_query_closest on device memory: every buffer is an integer device address (0 = none), `stream` a hipStream_t handle
        (0 = the null stream).  Asynchronous (include/tirt.h); ti_raytrace_amd.RayQuery is the torch front end."""
        check(lib().tirt_query_closest(self.handle, _vp(int(rays) or None), int(nr), int(ray_stride), int(stack_size), int(flags),
                                       _vp(int(out_t) or None), _vp(int(out_prim) or None), _vp(int(out_hit) or None), int(hit_stride),
                                       _vp(int(counts) or None), _vp(int(stream) or None)))

    def query_occluded(self, rays, nr, ray_stride, out_occluded, tmax=0, tmax_stride=1, tmax_all=float("inf"), stack_size=64, flags=0, stream=0):
        """tirt_query_occluded on device memory: integer device addresses, tmax = 0 means tmax_all for every ray."""
        check(lib().tirt_query_occluded(self.handle, _vp(int(rays) or None), int(nr), int(ray_stride), _vp(int(tmax) or None), int(tmax_stride),
                                        float(tmax_all), int(stack_size), int(flags), _vp(int(out_occluded) or None), _vp(int(stream) or None)))

    def query_hits(self, rays, nr, ray_stride, k, stack_size=64, flags=0, tmax=0, tmax_stride=1, tmax_all=float("inf"), out_t=0, out_prim=0, out_hit=0,
                   hit_stride=13, out_count=0, counts=0, stream=0):
        """tirt_query_hits on device memory (include/tirt.h, "First K hits"): every buffer is an integer device address (0 = none), tmax = 0 means
        tmax_all for every ray.  Asynchronous; ti_raytrace_amd.RayQuery.hits / .count are the torch front end."""
        check(lib().tirt_query_hits(self.handle, _vp(int(rays) or None), int(nr), int(ray_stride), _vp(int(tmax) or None), int(tmax_stride), float(tmax_all),
                                    int(k), int(stack_size), int(flags), _vp(int(out_t) or None), _vp(int(out_prim) or None), _vp(int(out_hit) or None),
                                    int(hit_stride), _vp(int(out_count) or None), _vp(int(counts) or None), _vp(int(stream) or None)))

    def trace_hits(self, rays, k, tmax=None, stack_size=64, flags=0, attributes=False, count=True):
        """tirt_trace_hits, the host route: rays (n, 6) float32, tmax None (= inf), a float or (n,) float32 ->
        (t (n, k), prim (n, k), record (n, k, 13) or None, count (n,) or None, counts (n, 2) or None [COUNT_NODES])"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n, k = rays.shape[0], int(k)
        bound = _bound(tmax, n)
        t = np.zeros((n, max(k, 0)), np.float32)
        prim = np.zeros((n, max(k, 0)), np.int32)
        rec = np.zeros((n, max(k, 0), 13), np.float32) if attributes else None
        cnt = np.zeros(n, np.int32) if count else None
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_trace_hits(self.handle, rays.reshape(-1), n, _ptr(bound), k, int(stack_size), int(flags), _ptr(t), _ptr(prim), _ptr(rec),
                                    _ptr(cnt), _ptr(counts)))
        return t, prim, rec, cnt, counts

    def query_closest_point(self, points, n, point_stride, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"), out_d2=0, out_prim=0,
                            out_point=0, point_out_stride=3, out_uv=0, uv_stride=2, counts=0, stream=0):
        """tirt_query_closest_point on device memory: every buffer is an integer device address (0 = none), dmax = 0 means dmax_all for every
        query.  Asynchronous (include/tirt.h, "Closest point"); ti_raytrace_amd.PointQuery is the torch front end."""
        check(lib().tirt_query_closest_point(self.handle, _vp(int(points) or None), int(n), int(point_stride), _vp(int(dmax) or None), int(dmax_stride),
                                             float(dmax_all), int(stack_size), int(flags), _vp(int(out_d2) or None), _vp(int(out_prim) or None),
                                             _vp(int(out_point) or None), int(point_out_stride), _vp(int(out_uv) or None), int(uv_stride),
                                             _vp(int(counts) or None), _vp(int(stream) or None)))

    def closest_point(self, points, max_distance=None, stack_size=64, flags=0, attributes=True):
        """tirt_closest_point, the host route: points (n, 3) float32, max_distance None (= inf), a float or (n,) float32 ->
        (dist2 (n,), prim (n,), point (n, 3) or None, uv (n, 2) or None, counts (n, 2) or None [COUNT_NODES])"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = points.shape[0]
        dmax = _bound(max_distance, n)
        d2 = np.zeros(n, np.float32)
        prim = np.zeros(n, np.int32)
        point = np.zeros((n, 3), np.float32) if attributes else None
        uv = np.zeros((n, 2), np.float32) if attributes else None
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_closest_point(self.handle, points.reshape(-1), n, _ptr(dmax), int(stack_size), int(flags), _ptr(d2), _ptr(prim),
                                       _ptr(point), _ptr(uv), _ptr(counts)))
        return d2, prim, point, uv, counts

    def query_nearest(self, points, n, point_stride, k, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"), out_d2=0, out_prim=0,
                      out_point=0, point_out_stride=3, out_uv=0, uv_stride=2, out_count=0, counts=0, stream=0):
        """tirt_query_nearest on device memory (include/tirt.h, "K nearest primitives"): every buffer is an integer device address (0 = none), dmax = 0
        means dmax_all for every query.  Asynchronous; ti_raytrace_amd.PointQuery.nearest / .count_within are the torch front end."""
        check(lib().tirt_query_nearest(self.handle, _vp(int(points) or None), int(n), int(point_stride), _vp(int(dmax) or None), int(dmax_stride),
                                       float(dmax_all), int(k), int(stack_size), int(flags), _vp(int(out_d2) or None), _vp(int(out_prim) or None),
                                       _vp(int(out_point) or None), int(point_out_stride), _vp(int(out_uv) or None), int(uv_stride),
                                       _vp(int(out_count) or None), _vp(int(counts) or None), _vp(int(stream) or None)))

    def nearest(self, points, k, max_distance=None, stack_size=64, flags=0, attributes=True, count=True):
        """tirt_nearest, the host route: points (n, 3) float32, max_distance None (= inf), a float or (n,) float32 ->
        (dist2 (n, k), prim (n, k), point (n, k, 3) or None, uv (n, k, 2) or None, count (n,) or None, counts (n, 2) or None [COUNT_NODES])"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n, k = points.shape[0], int(k)
        dmax = _bound(max_distance, n)
        d2 = np.zeros((n, max(k, 0)), np.float32)
        prim = np.zeros((n, max(k, 0)), np.int32)
        point = np.zeros((n, max(k, 0), 3), np.float32) if attributes else None
        uv = np.zeros((n, max(k, 0), 2), np.float32) if attributes else None
        cnt = np.zeros(n, np.int32) if count else None
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_nearest(self.handle, points.reshape(-1), n, _ptr(dmax), k, int(stack_size), int(flags), _ptr(d2), _ptr(prim), _ptr(point),
                                 _ptr(uv), _ptr(cnt), _ptr(counts)))
        return d2, prim, point, uv, cnt, counts

    def query_mesh_distance(self, tris, n, tri_stride, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"), out_d2=0, out_prim=0,
                            out_code=0, out_points=0, points_stride=6, counts=0, stream=0):
        """tirt_query_mesh_distance on device memory (include/tirt.h, "Triangle distance"): every buffer is an integer device address (0 = none), dmax = 0
        means dmax_all for every query.  Asynchronous; ti_raytrace_amd.TriangleQuery is the torch front end."""
        check(lib().tirt_query_mesh_distance(self.handle, _vp(int(tris) or None), int(n), int(tri_stride), _vp(int(dmax) or None), int(dmax_stride),
                                             float(dmax_all), int(stack_size), int(flags), _vp(int(out_d2) or None), _vp(int(out_prim) or None),
                                             _vp(int(out_code) or None), _vp(int(out_points) or None), int(points_stride),
                                             _vp(int(counts) or None), _vp(int(stream) or None)))

    def mesh_distance(self, tris, max_distance=None, stack_size=64, flags=0, points=True):
        """tirt_mesh_distance, the host route: tris (n, 3, 3) float32, max_distance None (= inf), a float or (n,) float32 ->
        (dist2 (n,), prim (n,), code (n,), points (n, 2, 3) [P on the query triangle, Q on the scene] or None, counts (n, 2) or None [COUNT_NODES])"""
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        n = tris.shape[0]
        dmax = _bound(max_distance, n)
        d2 = np.zeros(n, np.float32)
        prim = np.zeros(n, np.int32)
        code = np.zeros(n, np.int32)
        pq = np.zeros((n, 2, 3), np.float32) if points else None
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_mesh_distance(self.handle, tris.reshape(-1), n, _ptr(dmax), int(stack_size), int(flags), _ptr(d2), _ptr(prim), _ptr(code),
                                       _ptr(pq), _ptr(counts)))
        return d2, prim, code, pq, counts

    def query_point_pairs(self, points, n, point_stride, mode, row_start, capacity=0, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"),
                          out_d2=0, out_prim=0, out_point=0, point_out_stride=3, out_uv=0, uv_stride=2, counts=0, stream=0):
        """tirt_query_point_pairs on device memory (include/tirt.h, "Point pairs"): every buffer is an integer device address (0 = none), dmax = 0 means
        dmax_all for every query; mode is PAIRS_COUNT, PAIRS_FILL or PAIRS_BOTH.  Asynchronous; ti_raytrace_amd.PointQuery.within is the torch front end."""
        check(lib().tirt_query_point_pairs(self.handle, _vp(int(points) or None), int(n), int(point_stride), _vp(int(dmax) or None), int(dmax_stride),
                                           float(dmax_all), int(mode), int(capacity), int(stack_size), int(flags), _vp(int(row_start) or None),
                                           _vp(int(out_d2) or None), _vp(int(out_prim) or None), _vp(int(out_point) or None), int(point_out_stride),
                                           _vp(int(out_uv) or None), int(uv_stride), _vp(int(counts) or None), _vp(int(stream) or None)))

    def query_mesh_pairs(self, tris, n, tri_stride, mode, row_start, capacity=0, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"),
                         out_d2=0, out_prim=0, out_code=0, out_points=0, points_stride=6, counts=0, stream=0):
        """tirt_query_mesh_pairs on device memory (include/tirt.h, "Triangle pairs"), as query_point_pairs.  ti_raytrace_amd.TriangleQuery.pairs is the
        torch front end."""
        check(lib().tirt_query_mesh_pairs(self.handle, _vp(int(tris) or None), int(n), int(tri_stride), _vp(int(dmax) or None), int(dmax_stride),
                                          float(dmax_all), int(mode), int(capacity), int(stack_size), int(flags), _vp(int(row_start) or None),
                                          _vp(int(out_d2) or None), _vp(int(out_prim) or None), _vp(int(out_code) or None), _vp(int(out_points) or None),
                                          int(points_stride), _vp(int(counts) or None), _vp(int(stream) or None)))

    def _pairs_host(self, tri, query, max_distance, capacity, stack_size, flags, attributes):
        """the host routes of the pair lists: capacity None = a COUNT call, exact arrays, a FILL call; else one BOTH call into arrays of `capacity` pairs
        (pre-filled: -1 / NaN where no row was written)"""
        width = 9 if tri else 3
        query = np.ascontiguousarray(query, np.float32).reshape(-1, width)
        n = query.shape[0]
        dmax = _bound(max_distance, n)
        row_start = np.zeros(n + 1, np.int64)
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None

        def call(mode, cap, d2, prim, code, a0, a1):
            if tri:
                check(lib().tirt_mesh_pairs(self.handle, _ptr(query), n, _ptr(dmax), mode, cap, int(stack_size), int(flags), _ptr(row_start), _ptr(d2),
                                            _ptr(prim), _ptr(code), _ptr(a0), _ptr(counts)))
            else:
                check(lib().tirt_point_pairs(self.handle, _ptr(query), n, _ptr(dmax), mode, cap, int(stack_size), int(flags), _ptr(row_start), _ptr(d2),
                                             _ptr(prim), _ptr(a0), _ptr(a1), _ptr(counts)))
        mode = PAIRS_BOTH
        if capacity is None:
            call(PAIRS_COUNT, 0, None, None, None, None, None)
            capacity, mode = int(row_start[-1]), PAIRS_FILL
        capacity = int(capacity)
        d2 = np.full(capacity, np.nan, np.float32)
        prim = np.full(capacity, -1, np.int32)
        code = np.full(capacity, -1, np.int32) if tri else None
        a0 = np.zeros((capacity, 2, 3) if tri else (capacity, 3), np.float32) if attributes else None
        a1 = np.zeros((capacity, 2), np.float32) if attributes and not tri else None
        call(mode, capacity, d2, prim, code, a0, a1)
        return row_start, d2, prim, code, a0, a1, counts

    def point_pairs(self, points, max_distance=None, capacity=None, stack_size=64, flags=0, attributes=True):
        """tirt_point_pairs, the host route: points (n, 3) float32, max_distance None (= inf), a float or (n,) float32 ->
        (row_start (n + 1,) int64, prim, dist2, point (., 3) or None, uv (., 2) or None, counts (n, 2) or None [COUNT_NODES])"""
        row_start, d2, prim, _, point, uv, counts = self._pairs_host(False, points, max_distance, capacity, stack_size, flags, attributes)
        return row_start, prim, d2, point, uv, counts

    def mesh_pairs(self, tris, max_distance=None, capacity=None, stack_size=64, flags=0, points=True):
        """tirt_mesh_pairs, the host route: tris (n, 3, 3) float32 -> (row_start (n + 1,) int64, prim, dist2, code, points (., 2, 3) [P on the query
        triangle, Q on the scene] or None, counts (n, 2) or None [COUNT_NODES])"""
        row_start, d2, prim, code, pq, _, counts = self._pairs_host(True, tris, max_distance, capacity, stack_size, flags, points)
        return row_start, prim, d2, code, pq, counts

    def kat_tri_tri(self, rows, what=0):
        """include/tirt.h, tirt_kat_tri_tri: what = 0: rows (n, 18) (T, a, b, c) -> (n, 8) d2, P3, Q3, code; 1: (n, 12) two segments -> (n, 3) s, t, d2;
        2: (n, 15) segment and triangle -> (n, 4) hit, u, v, t"""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_TRI_TRI_ROWS[what][0])
        out = np.zeros((rows.shape[0], KAT_TRI_TRI_ROWS[what][1]), np.float32)
        if rows.shape[0]:
            check(lib().tirt_kat_tri_tri(self.handle, rows.reshape(-1), rows.shape[0], int(what), out.reshape(-1)))
        return out

    def kat_closest_point(self, rows, is_sphere=False):
        """include/tirt.h, tirt_kat_closest_point: rows (n, 12) (p, a, b, c) or, is_sphere, (n, 7) (p, c, r) -> (n, 6): d2, q3, u, v"""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 7 if is_sphere else 12)
        out = np.zeros((rows.shape[0], 6), np.float32)
        check(lib().tirt_kat_closest_point(self.handle, rows.reshape(-1), rows.shape[0], 1 if is_sphere else 0, out.reshape(-1)))
        return out

    def query_sweep(self, rays, n, ray_stride, stack_size=64, flags=0, radius=0, radius_stride=1, radius_all=0.0, tmax=0, tmax_stride=1,
                    tmax_all=float("inf"), out_t=0, out_prim=0, out_code=0, out_point=0, point_stride=3, out_uv=0, uv_stride=2, out_normal=0,
                    normal_stride=3, out_blocked=0, counts=0, stream=0):
        """tirt_query_sweep on device memory (include/tirt.h, "Sphere sweep"): every buffer is an integer device address (0 = none), radius = 0 means
        radius_all and tmax = 0 means tmax_all for every query.  Asynchronous; ti_raytrace_amd.SweepQuery is the torch front end."""
        check(lib().tirt_query_sweep(self.handle, _vp(int(rays) or None), int(n), int(ray_stride), _vp(int(radius) or None), int(radius_stride),
                                     float(radius_all), _vp(int(tmax) or None), int(tmax_stride), float(tmax_all), int(stack_size), int(flags),
                                     _vp(int(out_t) or None), _vp(int(out_prim) or None), _vp(int(out_code) or None), _vp(int(out_point) or None),
                                     int(point_stride), _vp(int(out_uv) or None), int(uv_stride), _vp(int(out_normal) or None), int(normal_stride),
                                     _vp(int(out_blocked) or None), _vp(int(counts) or None), _vp(int(stream) or None)))

    def sweep(self, rays, radius, tmax=None, stack_size=64, flags=0, attributes=True, blocked_only=False):
        """tirt_sweep, the host route: rays (n, 6) float32, radius a float or (n,) float32, tmax None (= inf), a float or (n,) float32 ->
        a dict of t (n,), prim (n,), code (n,), point (n, 3), uv (n, 2), normal (n, 3) [attributes], blocked (n,) bool, counts (n, 2) [COUNT_NODES];
        blocked_only: `blocked` (and counts) alone, through the walk that stops at the first contact"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        rad = _bound(radius, n)
        bound = _bound(tmax, n)
        out = {"blocked": np.zeros(n, np.uint8)}
        if not blocked_only:
            out.update(t=np.zeros(n, np.float32), prim=np.zeros(n, np.int32), code=np.zeros(n, np.int32))
            if attributes:
                out.update(point=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32), normal=np.zeros((n, 3), np.float32))
        if flags & COUNT_NODES:
            out["counts"] = np.zeros((n, 2), np.int32)
        check(lib().tirt_sweep(self.handle, rays.reshape(-1), n, _ptr(rad), 0.0, _ptr(bound), int(stack_size), int(flags), _ptr(out.get("t")),
                               _ptr(out.get("prim")), _ptr(out.get("code")), _ptr(out.get("point")), _ptr(out.get("uv")), _ptr(out.get("normal")),
                               _ptr(out["blocked"]), _ptr(out.get("counts"))))
        out["blocked"] = out["blocked"].view(np.bool_)
        return out

    def kat_sweep(self, rows, is_sphere=False):
        """include/tirt.h, tirt_kat_sweep: rows (n, 18) (o, d, r, m, B, a, b, c) or, is_sphere, (n, 13) (o, d, r, m, B, C, R) -> (n, 8): T, code, Q3, u, v, D2"""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_SWEEP_ROWS[bool(is_sphere)])
        out = np.zeros((rows.shape[0], 8), np.float32)
        if rows.shape[0]:
            check(lib().tirt_kat_sweep(self.handle, rows.reshape(-1), rows.shape[0], 1 if is_sphere else 0, out.reshape(-1)))
        return out

    def query_signed_distance(self, points, n, point_stride, out_sd, stack_size=64, flags=0, dmax=0, dmax_stride=1, dmax_all=float("inf"), out_d2=0,
                              out_prim=0, out_point=0, point_out_stride=3, out_uv=0, uv_stride=2, counts=0, stream=0):
        """tirt_query_signed_distance on device memory (include/tirt.h, "Signed distance"): query_closest_point with out_sd; the first call after the
        geometry changed builds the pseudo-normal table on the context's stream.  ti_raytrace_amd.PointQuery is the torch front end."""
        check(lib().tirt_query_signed_distance(self.handle, _vp(int(points) or None), int(n), int(point_stride), _vp(int(dmax) or None), int(dmax_stride),
                                               float(dmax_all), int(stack_size), int(flags), _vp(int(out_d2) or None), _vp(int(out_prim) or None),
                                               _vp(int(out_point) or None), int(point_out_stride), _vp(int(out_uv) or None), int(uv_stride),
                                               _vp(int(counts) or None), _vp(int(stream) or None), _vp(int(out_sd) or None)))

    def signed_distance(self, points, max_distance=None, stack_size=64, flags=0, attributes=True):
        """tirt_signed_distance, the host route: as closest_point, with the signed distance first ->
        (dist (n,), dist2 (n,), prim (n,), point (n, 3) or None, uv (n, 2) or None, counts (n, 2) or None [COUNT_NODES])"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = points.shape[0]
        dmax = _bound(max_distance, n)
        sd = np.zeros(n, np.float32)
        d2 = np.zeros(n, np.float32)
        prim = np.zeros(n, np.int32)
        point = np.zeros((n, 3), np.float32) if attributes else None
        uv = np.zeros((n, 2), np.float32) if attributes else None
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_signed_distance(self.handle, points.reshape(-1), n, _ptr(dmax), int(stack_size), int(flags), _ptr(d2), _ptr(prim),
                                         _ptr(point), _ptr(uv), _ptr(counts), _ptr(sd)))
        return sd, d2, prim, point, uv, counts

    def signed_distance_prepare(self):
        """tirt_signed_distance_prepare: builds the table now and waits -> the five counts as a dict, and `closed` (the first four are zero)"""
        out = (C.c_int64 * 5)()
        check(lib().tirt_signed_distance_prepare(self.handle, out))
        r = dict(zip(SD_REPORT, (int(x) for x in out)))
        r["closed"] = not any(r[k] for k in SD_REPORT[:4])
        return r

    def signed_distance_table(self):
        """tirt_signed_distance_table_download: (n, 7, 4) float32 -- rows interior, A, B, C, AB, AC, BC; [:, 0, 3] viewed as int32 holds the edge classes"""
        n = self.signed_distance_prepare()["primitives"]
        out = np.zeros((n, 7, 4), np.float32)
        check(lib().tirt_signed_distance_table_download(self.handle, out.reshape(-1)))
        return out

    def kat_signed_distance(self, rows):
        """include/tirt.h, tirt_kat_signed_distance: rows (n, 33) (p, a, b, c, N[7][3]) -> (n, 2): sd, the feature's row index"""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 33)
        out = np.zeros((rows.shape[0], 2), np.float32)
        check(lib().tirt_kat_signed_distance(self.handle, rows.reshape(-1), rows.shape[0], out.reshape(-1)))
        return out

    def query_winding_number(self, points, n, point_stride, out_w, beta=2.0, stack_size=64, flags=0, counts=0, stream=0):
        """tirt_query_winding_number on device memory (include/tirt.h, "Winding number"); the first call after the geometry changed builds the moment
        table on the context's stream.  ti_raytrace_amd.PointQuery is the torch front end."""
        check(lib().tirt_query_winding_number(self.handle, _vp(int(points) or None), int(n), int(point_stride), float(beta), int(stack_size), int(flags),
                                              _vp(int(out_w) or None), _vp(int(counts) or None), _vp(int(stream) or None)))

    def winding_number(self, points, beta=2.0, stack_size=64, flags=0):
        """tirt_winding_number, the host route: points (n, 3) -> w (n,) float32, or (w, counts (n, 2) int32) with COUNT_NODES"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = points.shape[0]
        w = np.zeros(n, np.float32)
        counts = np.zeros((n, 2), np.int32) if (flags & COUNT_NODES) else None
        check(lib().tirt_winding_number(self.handle, points.reshape(-1), n, float(beta), int(stack_size), int(flags), _ptr(w), _ptr(counts)))
        return (w, counts) if counts is not None else w

    def winding_prepare(self):
        """tirt_winding_prepare: builds the moment table now (unless it stands) and waits"""
        check(lib().tirt_winding_prepare(self.handle))

    def winding_table(self):
        """tirt_winding_table_download -> (table (wide_nodes, 4, 16) float32: per node and child slot p~ 3, r2, N 3, C 9; sums (wide_nodes, 16) int64: the
        integer moments of everything beneath each node; e: the exponent of the scales)"""
        info = np.zeros(2, np.int32)
        check(lib().tirt_winding_table_download(self.handle, None, None, _ptr(info)))
        table = np.zeros((int(info[0]), 4, 16), np.float32); sums = np.zeros((int(info[0]), 16), np.int64)
        check(lib().tirt_winding_table_download(self.handle, _ptr(table), _ptr(sums), _ptr(info)))
        return table, sums, int(info[1])

    def kat_winding(self, rows, is_sphere=False):
        """include/tirt.h, tirt_kat_winding: rows (n, 12) (q, A, B, C) or (n, 7) (q, centre, r) -> (omega (n,) float32, w (n,) float32, I (n,) int64)"""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_WINDING_ROWS[bool(is_sphere)])
        out = np.zeros((rows.shape[0], 4), np.uint32)
        if rows.shape[0]:
            check(lib().tirt_kat_winding(self.handle, rows.reshape(-1), rows.shape[0], 1 if is_sphere else 0, _ptr(out)))
        return _kat_winding_out(out)

    def bvh_info(self):
        out = (C.c_uint64 * 4)()
        check(lib().tirt_bvh_info(self.handle, out))
        return {"node_bytes": int(out[0]), "prim_bytes": int(out[1]), "nodes": int(out[2]), "nodes_in_lds": int(out[3])}

    def trace_timeline(self, max_waves=1 << 16):
        """Per-wave [start, queue empty, end, hw id] of the launch armed by set_option("trace_timeline", k): (n, 4) uint64."""
        import numpy as np
        out = np.zeros((max_waves, 4), np.uint64); n = C.c_int(0)
        check(lib().tirt_trace_timeline(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(max_waves), C.byref(n)))
        return out[:min(n.value, max_waves)]

    def primary_beam_stats(self):
        """Diagnostics of the camera rays' candidate lists (tirt.h, tirt_primary_beam_stats)."""
        out = (C.c_uint64 * 12)()
        check(lib().tirt_primary_beam_stats(self.handle, out))
        return {"pixels_with_list": int(out[0]), "leaves_listed": int(out[1]), "pixels_all_probes_hit": int(out[2]), "rays_to_k_trace": int(out[3]), "rays": int(out[4]),
                "list_builds": int(out[5]), "list_build_ms": out[6] * 1.0e-6, "list_builds_skipped": int(out[7]),
                "diag_leaf_steps": int(out[8]), "diag_rays_more_than_one_step": int(out[9]), "diag_lane_slots": int(out[10]), "diag_rays_more_than_two_steps": int(out[11])}

    def primary_beam_lists_info(self):
        """tirt.h, tirt_primary_beam_lists_download with NULL arrays: {"P", "cmax", "lists" (bool), "pixels_with_list"}"""
        info = np.zeros(4, np.int32)
        check(lib().tirt_primary_beam_lists_download(self.handle, None, None, None, _ptr(info)))
        return {"P": int(info[0]), "cmax": int(info[1]), "lists": bool(info[2]), "pixels_with_list": int(info[3])}

    def primary_beam_lists_download(self):
        """The camera rays' candidate lists of the current (build, camera, film), made first if they do not stand (tirt.h, tirt_primary_beam_lists_download): the
        info above and, in local pixel order, count int32 [P], code int32 [cmax, P] (the leaves' child codes), nr float32 [cmax, P], bound float32 [P]."""
        out = self.primary_beam_lists_info()
        P, cmax = out["P"], out["cmax"]
        count = np.zeros(P, np.int32); cand = np.zeros((cmax, P, 2), np.int32); bound = np.zeros(P, np.float32)
        info = np.zeros(4, np.int32)
        check(lib().tirt_primary_beam_lists_download(self.handle, _ptr(count), _ptr(cand), _ptr(bound), _ptr(info)))
        out.update(lists=bool(info[2]), pixels_with_list=int(info[3]), count=count, code=np.ascontiguousarray(cand[:, :, 0]),
                   nr=np.ascontiguousarray(cand[:, :, 1]).view(np.float32), bound=bound)
        return out

    def kat_primary_list_walk(self, local_pixel, jx, jy, out_stride=KAT_LIST_WALK_OUT):
        """tirt.h, tirt_kat_primary_list_walk: rows (local pixel, jx, jy) -> (n, out_stride) float32: d3, resolved, t, u, v, prim (bits), steps.  Row r runs on lane
        r % 64 of wave r // 64."""
        local_pixel = np.ascontiguousarray(local_pixel, np.int32).reshape(-1)
        jx = np.ascontiguousarray(jx, np.float32).reshape(-1); jy = np.ascontiguousarray(jy, np.float32).reshape(-1)
        n = local_pixel.shape[0]
        if jx.shape[0] != n or jy.shape[0] != n:
            raise ValueError("kat_primary_list_walk: local_pixel, jx and jy have one entry per row")
        out = np.zeros((n, out_stride), np.float32)
        check(lib().tirt_kat_primary_list_walk(self.handle, n, local_pixel, jx, jy, out.reshape(-1), int(out_stride)))
        return out

    def micro_gather_rate(self, working_set_bytes, iters=2000):
        v = C.c_double(0.0)
        check(lib().tirt_micro_gather_rate(self.handle, int(working_set_bytes), int(iters), C.byref(v)))
        return float(v.value)

    def stats(self):
        st = Stats()
        rc = lib().tirt_stats(self.handle, C.byref(st))
        if rc == ERR_STACK:
            msg = lib().tirt_last_error()
            raise TirtStackOverflow("libtirt error %d: %s" % (rc, msg.decode() if msg else "?"), st.as_dict())
        check(rc)
        return st.as_dict()

    def stats_reset(self):
        check(lib().tirt_stats_reset(self.handle))

    def kat_math(self, fn, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), np.float32)
        out = np.zeros_like(x)
        check(lib().tirt_kat_math(self.handle, int(fn), x, y, out, x.size))
        return out

    def kat_brdf(self, which, inp, out_stride):
        return _kat_rows("tirt_kat_brdf", self.handle, (int(which),), inp, out_stride)

    def shade_table_download(self, which, count):
        """The shading records (which 0, count = primitives) or the light records (which 1, count = light_count): (count, 8, 4) float32."""
        out = np.zeros((int(count), 8, 4), np.float32)
        check(lib().tirt_shade_table_download(self.handle, int(which), out.reshape(-1), out.size))
        return out

    def kat_shade_tables(self, which, n, inp=None):
        """include/tirt.h, tirt_kat_shade_tables: (n, 4), (n, 5) or -- which 2, inp (n, 6) -- (n, 2, 12) float32."""
        if inp is not None:
            inp = np.ascontiguousarray(inp, np.float32)
            n = inp.shape[0]
        out = np.zeros((int(n), 4) if which == 0 else (int(n), 5) if which == 1 else (int(n), 2, 12), np.float32)
        check(lib().tirt_kat_shade_tables(self.handle, int(which), _ptr(inp), out.reshape(-1), int(n)))
        return out

    def kat_shade_step(self, feat, rows, out_stride=KAT_STEP_OUT):
        """include/tirt.h, tirt_kat_shade_step: rows (n, >= 23) of 32-bit words (float32 view; integers as bit patterns) -> (n, out_stride) float32."""
        return kat_shade_step(self.handle, feat, rows, out_stride)

    def kat_shade_spec_step(self, feat, rows, out_stride=KAT_SPEC_STEP_OUT):
        """include/tirt.h, tirt_kat_shade_spec_step: rows (n, >= 23) of 32-bit words (float32 view; integers as bit patterns) -> (n, out_stride) float32."""
        return kat_shade_spec_step(self.handle, feat, rows, out_stride)

    def kat_spec(self, which, inp, out_stride):
        return _kat_rows("tirt_kat_spec", self.handle, (int(which),), inp, out_stride)


def kat_shade_step(handle, feat, rows, out_stride=KAT_STEP_OUT, in_stride=None):
    """tirt_kat_shade_step on a raw context handle (None: only the refusals that need no context can be reached)."""
    return _kat_rows("tirt_kat_shade_step", handle, (int(feat),), rows, out_stride, words=True, in_stride=in_stride)


def kat_shade_spec_step(handle, feat, rows, out_stride=KAT_SPEC_STEP_OUT, in_stride=None):
    """tirt_kat_shade_spec_step on a raw context handle (None: only the refusals that need no context can be reached)."""
    return _kat_rows("tirt_kat_shade_spec_step", handle, (int(feat),), rows, out_stride, words=True, in_stride=in_stride)


def texture_upload(handle, textures):
    """tirt_texture_upload on a raw context handle (None: only the refusals that need no context can be reached): the textures packed back to back"""
    imgs = [np.ascontiguousarray(img, np.int32) for img, _ in textures]
    for img in imgs:
        if img.ndim != 2:
            raise ValueError("texture_upload: a texture is a [w, h] array of packed texels (Texture.np_img), got shape %s" % (img.shape,))
    n = len(imgs)
    w = np.asarray([img.shape[0] for img in imgs], np.int32)
    h = np.asarray([img.shape[1] for img in imgs], np.int32)
    wrap = np.asarray([int(wr) for _, wr in textures], np.int32)
    sizes = np.asarray([img.size for img in imgs], np.int64)
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    texels = np.concatenate([img.reshape(-1) for img in imgs]) if n else np.zeros(0, np.int32)
    check(lib().tirt_texture_upload(handle, n, _ptr(texels) if n else None, int(texels.size), _ptr(offset) if n else None,
                                    _ptr(w) if n else None, _ptr(h) if n else None, _ptr(wrap) if n else None))


def texture_cutout(handle, flags, count=None):
    """tirt_texture_cutout on a raw context handle (None: only the refusals that need no context can be reached)"""
    flags = np.ascontiguousarray(flags, np.int32).reshape(-1)
    check(lib().tirt_texture_cutout(handle, _ptr(flags) if flags.size else None, int(flags.size if count is None else count)))


def shade_instantiation(word, specialize=True, spectral=False):
    """include/tirt.h, tirt_shade_instantiation: the word of the instantiation of k_shade (spectral: k_shade_spec) a render launches for a feature word; needs no device."""
    out = C.c_uint32(0)
    check(lib().tirt_shade_instantiation(int(word), int(specialize), int(spectral), C.byref(out)))
    return int(out.value)


def kat_hit_list(cand, k, bound=float("inf")):
    """include/tirt.h, tirt_kat_hit_list (host only, no context): cand (n, 4) words (t, u, v as float32 bits, leaf as int32), in the order given, through the
    list code of csrc/tirt_multi_hit.h -> (list (held, 4) words, candidates with 0 < t < B, (threshold t, threshold leaf))"""
    cand = np.ascontiguousarray(cand).view(np.float32).reshape(-1, 4)
    out = np.zeros((max(int(k), 0), 4), np.float32)
    info = np.zeros(4, np.int32)
    check(lib().tirt_kat_hit_list(cand.reshape(-1), cand.shape[0], int(k), float(bound), _ptr(out), info))
    return out[:info[0]].copy(), int(info[1]), (float(info[2:3].view(np.float32)[0]), int(info[3]))


KAT_TRI_TRI_ROWS = {0: (18, 8), 1: (12, 3), 2: (15, 4)}             # tirt_kat_tri_tri[_host]: floats per input and output row of each `what`


def kat_tri_tri_host(rows, what=0):
    """include/tirt.h, tirt_kat_tri_tri_host (host only, no context): Context.kat_tri_tri's rows through the same text compiled for the host"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_TRI_TRI_ROWS[what][0])
    out = np.zeros((rows.shape[0], KAT_TRI_TRI_ROWS[what][1]), np.float32)
    if rows.shape[0]:
        check(lib().tirt_kat_tri_tri_host(rows.reshape(-1), rows.shape[0], int(what), out.reshape(-1)))
    return out


KAT_WINDING_ROWS = {False: 12, True: 7}                             # tirt_kat_winding[_host]: floats per input row of a triangle / an analytic sphere


def _kat_winding_out(out):
    return out[:, 0].copy().view(np.float32), out[:, 1].copy().view(np.float32), np.ascontiguousarray(out[:, 2:4]).view(np.int64).reshape(-1)


def kat_winding_host(rows, is_sphere=False):
    """include/tirt.h, tirt_kat_winding_host (host only, no context): Context.kat_winding's rows through the same text compiled for the host"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_WINDING_ROWS[bool(is_sphere)])
    out = np.zeros((rows.shape[0], 4), np.uint32)
    if rows.shape[0]:
        check(lib().tirt_kat_winding_host(rows.reshape(-1), rows.shape[0], 1 if is_sphere else 0, _ptr(out)))
    return _kat_winding_out(out)


KAT_SWEEP_ROWS = {False: 18, True: 13}                              # tirt_kat_sweep[_host]: floats per input row of a triangle / an analytic sphere


def kat_sweep_host(rows, is_sphere=False):
    """include/tirt.h, tirt_kat_sweep_host (host only, no context): Context.kat_sweep's rows through the same text compiled for the host"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, KAT_SWEEP_ROWS[bool(is_sphere)])
    out = np.zeros((rows.shape[0], 8), np.float32)
    if rows.shape[0]:
        check(lib().tirt_kat_sweep_host(rows.reshape(-1), rows.shape[0], 1 if is_sphere else 0, out.reshape(-1)))
    return out


def kat_beam_triangle_host(rows, edges=1):
    """include/tirt.h, tirt_kat_beam_triangle_host (host only, no context): rows (n, 31) = eye, cell, the pyramid's four corner directions, eps, the
    triangle's corners -> (n,) int32, 1 = off (the list build would not list the leaf); edges = 0: the four faces alone"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 31)
    out = np.zeros(rows.shape[0], np.int32)
    if rows.shape[0]:
        check(lib().tirt_kat_beam_triangle_host(rows.reshape(-1), rows.shape[0], int(edges), out))
    return out


def kat_nearest_list(d2, prim, k, lim2=float("inf")):
    """include/tirt.h, tirt_kat_nearest_list (host only, no context): candidates (d2 (n,) float32, prim (n,) int32), in the order given, through the list code
    of csrc/tirt_nearest.h -> (d2 (k,), prim (k,) padded with (inf, -1), entries held, |N|, (threshold d2, threshold prim))"""
    d2 = np.ascontiguousarray(d2, np.float32).reshape(-1)
    prim = np.ascontiguousarray(prim, np.int32).reshape(-1)
    assert d2.shape == prim.shape
    out_d2 = np.zeros(max(int(k), 0), np.float32)
    out_prim = np.zeros(max(int(k), 0), np.int32)
    info = np.zeros(4, np.int32)
    check(lib().tirt_kat_nearest_list(_ptr(d2) if d2.size else None, _ptr(prim) if prim.size else None, d2.shape[0], int(k), float(lim2),
                                      _ptr(out_d2) if out_d2.size else None, _ptr(out_prim) if out_prim.size else None, info))
    return out_d2, out_prim, int(info[0]), int(info[1]), (float(info[2:3].view(np.float32)[0]), int(info[3]))


def kat_pairs_host(d2, prim, row_len, capacity=None, fill=(np.nan, -1)):
    """include/tirt.h, tirt_kat_pairs_host (host only, no context): rows of members (d2, prim) -- row i is the next row_len[i] entries -- in the order
    given, through the scan, the capacity rule and the sorting network of csrc/tirt_pairs.h -> (row_start (rows + 1,) int64, d2 (capacity,), prim
    (capacity,)): the rows that fit in order, `fill` elsewhere.  capacity None = the total"""
    d2 = np.ascontiguousarray(d2, np.float32).reshape(-1)
    prim = np.ascontiguousarray(prim, np.int32).reshape(-1)
    row_len = np.ascontiguousarray(row_len, np.int32).reshape(-1)
    assert d2.shape == prim.shape and int(row_len.sum()) == d2.shape[0]
    capacity = d2.shape[0] if capacity is None else int(capacity)
    row_start = np.zeros(row_len.shape[0] + 1, np.int64)
    out_d2 = np.full(max(capacity, 0), fill[0], np.float32)
    out_prim = np.full(max(capacity, 0), fill[1], np.int32)
    check(lib().tirt_kat_pairs_host(_ptr(d2) if d2.size else None, _ptr(prim) if prim.size else None, _ptr(row_len) if row_len.size else None,
                                    row_len.shape[0], capacity, _ptr(row_start), _ptr(out_d2) if out_d2.size else None,
                                    _ptr(out_prim) if out_prim.size else None))
    return row_start, out_d2, out_prim


def shade_features_host(material, primitive, shape, light, light_count, env=None, env_power=0.0):
    """The scene feature word of host tables (Scene.material_np, primitive_np, shape_np, light_np, light_count, Texture.np_img): needs no device."""
    material = np.ascontiguousarray(material, np.float32); primitive = np.ascontiguousarray(primitive, np.int32)
    shape = np.ascontiguousarray(shape, np.float32); light = np.ascontiguousarray(light, np.int32)
    env = None if env is None else np.ascontiguousarray(env, np.int32)
    out = C.c_uint32(0)
    check(lib().tirt_shade_features_host(material.reshape(-1), material.shape[0], primitive.reshape(-1), primitive.shape[0], shape.reshape(-1), shape.shape[0],
                                         light.reshape(-1), int(light_count), _ptr(env), 0 if env is None else env.shape[0], 0 if env is None else env.shape[1],
                                         float(env_power), C.byref(out)))
    return int(out.value)


def shade_features_host_env(material, primitive, shape, light, light_count, env=None, env_power=0.0, env_sampling=False):
    """shade_features_host with the switch of tirt_env_sampling as an input: bit 1024 where a context would report it."""
    material = np.ascontiguousarray(material, np.float32); primitive = np.ascontiguousarray(primitive, np.int32)
    shape = np.ascontiguousarray(shape, np.float32); light = np.ascontiguousarray(light, np.int32)
    env = None if env is None else np.ascontiguousarray(env, np.int32)
    out = C.c_uint32(0)
    check(lib().tirt_shade_features_host_env(material.reshape(-1), material.shape[0], primitive.reshape(-1), primitive.shape[0], shape.reshape(-1), shape.shape[0],
                                             light.reshape(-1), int(light_count), _ptr(env), 0 if env is None else env.shape[0], 0 if env is None else env.shape[1],
                                             float(env_power), 1 if env_sampling else 0, C.byref(out)))
    return int(out.value)


def shade_features_host_env_hdr(material, primitive, shape, light, light_count, env=None, env_power=0.0, env_sampling=False, env_format=0, dims=None):
    """shade_features_host_env with the texel format as an input (0 8-bit, 1 RGBE8): bits 2048 and 1024 where a context would report them.
    dims: (w, h) passed in place of env's shape (the refusals of w, h < 1)."""
    material = np.ascontiguousarray(material, np.float32); primitive = np.ascontiguousarray(primitive, np.int32)
    shape = np.ascontiguousarray(shape, np.float32); light = np.ascontiguousarray(light, np.int32)
    env = None if env is None else np.ascontiguousarray(env, np.int32)
    w, h = dims if dims is not None else ((0, 0) if env is None else env.shape)
    out = C.c_uint32(0)
    check(lib().tirt_shade_features_host_env_hdr(material.reshape(-1), material.shape[0], primitive.reshape(-1), primitive.shape[0], shape.reshape(-1), shape.shape[0],
                                                 light.reshape(-1), int(light_count), _ptr(env), int(w), int(h),
                                                 float(env_power), 1 if env_sampling else 0, int(env_format), C.byref(out)))
    return int(out.value)


def env_upload_hdr(handle, packed, power, dims=None):
    """tirt_env_upload_hdr on a raw context handle (None: only the refusals that need no context can be reached).  dims: (w, h) in place of packed's shape."""
    packed = None if packed is None else np.ascontiguousarray(packed, np.int32)
    w, h = dims if dims is not None else ((0, 0) if packed is None else packed.shape)
    check(lib().tirt_env_upload_hdr(handle, _ptr(packed), int(w), int(h), float(power)))


def shade_features_host_lights(material, primitive, shape, light, light_count, vertex=None, light_sampling=False, env=None, env_power=0.0, env_sampling=False, env_format=0):
    """shade_features_host_env_hdr with the mode of tirt_light_sampling as an input, and the vertex rows a triangle emitter's area needs: bit 4096 where a context would report it."""
    material = np.ascontiguousarray(material, np.float32); primitive = np.ascontiguousarray(primitive, np.int32)
    shape = np.ascontiguousarray(shape, np.float32); light = np.ascontiguousarray(light, np.int32)
    env = None if env is None else np.ascontiguousarray(env, np.int32)
    vertex = None if vertex is None else np.ascontiguousarray(vertex, np.float32)
    out = C.c_uint32(0)
    check(lib().tirt_shade_features_host_lights(material.reshape(-1), material.shape[0], primitive.reshape(-1), primitive.shape[0], shape.reshape(-1), shape.shape[0],
                                                light.reshape(-1), int(light_count), _ptr(env), 0 if env is None else env.shape[0], 0 if env is None else env.shape[1],
                                                float(env_power), 1 if env_sampling else 0, int(env_format), _ptr(vertex), 0 if vertex is None else vertex.shape[0],
                                                1 if light_sampling else 0, C.byref(out)))
    return int(out.value)


def light_sampling(handle, mode, uniform_share=0.0):
    """tirt_light_sampling on a raw context handle (None: only the refusals that need no context can be reached)"""
    check(lib().tirt_light_sampling(handle, int(mode), float(uniform_share)))


def env_sampling(handle, on, share=0.5):
    """tirt_env_sampling on a raw context handle (None: only the refusals that need no context can be reached)"""
    check(lib().tirt_env_sampling(handle, 1 if on else 0, float(share)))


def device_count():
    v = C.c_int(0)
    check(lib().tirt_device_count(C.byref(v)))
    return v.value


class Communicator:
    """RCCL communicator over several contexts of ONE process (tirt_comm_init / tirt_film_reduce)."""

    def __init__(self, contexts):
        self.contexts = list(contexts)
        self._arr = (C.c_void_p * len(self.contexts))(*[c.handle.value for c in self.contexts])
        check(lib().tirt_comm_init(self._arr, len(self.contexts)))

    def film_reduce(self, root=0):
        check(lib().tirt_film_reduce(self._arr, len(self.contexts), int(root)))

    def close(self):
        if self._arr is not None:
            lib().tirt_comm_destroy(self._arr, len(self.contexts))
            self._arr = None
