"""ctypes binding of libmifx.so (include/mifx.h). Device memory comes from torch tensors (plumbing only):
an image is a contiguous float32 CUDA tensor of shape (H, W) / (H, W, 2) / (H, W, 4).

There is NO CPU fallback here: if libmifx.so is missing, importing this module raises."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MIFX_STORAGE=h4 selects the RGBA16_FLOAT storage build of the library for the whole process (include/mifx.h: mifx_storage_mode); MIFX_LIB_PATH: an
# alternative build of the same library (the sanitizer build of the host objects)
STORAGE_H4 = os.environ.get("MIFX_STORAGE", "fp32").lower() in ("h4", "rgba16f", "f16")
LIB_PATH = os.environ.get("MIFX_LIB_PATH") or os.path.join(HERE, "libmifx_h4.so" if STORAGE_H4 else "libmifx.so")

MIFX_OK = 0
FORMAT_F32, FORMAT_F32X2, FORMAT_F32X4, FORMAT_F16X4 = 1, 2, 4, 8
FORMAT_U8, FORMAT_F16, FORMAT_F16X2, FORMAT_R11G11B10, FORMAT_U16 = 16, 32, 64, 128, 256  # the narrow planes of the native-storage build (include/mifx.h)
FORMAT_U16X2 = 512  # RG16_UNORM: the 16-bit filterable shadow map of SHADOW_MODE_VSM, in both builds

c_f = ctypes.c_float
c_i = ctypes.c_int32
c_u = ctypes.c_uint32
c_p = ctypes.c_void_p


class Image2D(ctypes.Structure):
    _fields_ = [("data", c_p), ("width", c_u), ("height", c_u), ("pitch_bytes", c_u), ("format", c_u)]


class Cubemap(ctypes.Structure):
    _fields_ = [("mip_data", c_p * 16), ("size", c_u), ("mip_count", c_u)]


class CameraAttribs(ctypes.Structure):
    _fields_ = [
        ("f4Position", c_f * 4), ("f4ViewportSize", c_f * 4),
        ("fNearPlaneZ", c_f), ("fFarPlaneZ", c_f), ("fNearPlaneDepth", c_f), ("fFarPlaneDepth", c_f),
        ("fSceneNearZ", c_f), ("fSceneFarZ", c_f), ("fSceneNearDepth", c_f), ("fSceneFarDepth", c_f),
        ("fHandness", c_f), ("uiFrameIndex", c_u), ("Padding0", c_f), ("Padding1", c_f),
        ("fFocusDistance", c_f), ("fFStop", c_f), ("fFocalLength", c_f), ("fSensorWidth", c_f),
        ("fSensorHeight", c_f), ("fExposure", c_f), ("f2Jitter", c_f * 2),
        ("mView", c_f * 16), ("mProj", c_f * 16), ("mViewProj", c_f * 16),
        ("mViewInv", c_f * 16), ("mProjInv", c_f * 16), ("mViewProjInv", c_f * 16),
        ("f4ExtraData", (c_f * 4) * 5),
    ]


class ToneMappingAttribs(ctypes.Structure):
    _fields_ = [
        ("iToneMappingMode", c_i), ("bAutoExposure", c_i), ("fMiddleGray", c_f), ("bLightAdaptation", c_i),
        ("fWhitePoint", c_f), ("fLuminanceSaturation", c_f), ("Padding0", c_u), ("Padding1", c_u),
        ("AgXSaturation", c_f), ("AgXSlope", c_f), ("AgXPower", c_f), ("AgXOffset", c_f),
    ]

    @classmethod
    def default(cls, mode=4):
        return cls(mode, 1, 0.18, 1, 3.0, 1.0, 0, 0, 1.0, 1.0, 1.0, 0.0)


class SSAOAttribs(ctypes.Structure):
    _fields_ = [
        ("EffectRadius", c_f), ("EffectFalloffRange", c_f), ("RadiusMultiplier", c_f), ("DepthMIPSamplingOffset", c_f),
        ("TemporalStabilityFactor", c_f), ("SpatialReconstructionRadius", c_f), ("ResetAccumulation", c_i), ("AlphaInterpolation", c_f),
        ("BitmaskThickness", c_f), ("Algorithm", c_u), ("Padding0", c_f), ("Padding1", c_f),
    ]

    @classmethod
    def default(cls):
        return cls(1.0, 0.615, 1.457, 3.3, 0.9, 4.0, 0, 1.0, 0.5, 0, 0.0, 0.0)


class SSRAttribs(ctypes.Structure):
    _fields_ = [
        ("DepthBufferThickness", c_f), ("RoughnessThreshold", c_f), ("MostDetailedMip", c_u), ("IsRoughnessPerceptual", c_i),
        ("RoughnessChannel", c_u), ("MaxTraversalIntersections", c_u), ("GGXImportanceSampleBias", c_f), ("SpatialReconstructionRadius", c_f),
        ("TemporalRadianceStabilityFactor", c_f), ("TemporalVarianceStabilityFactor", c_f), ("BilateralCleanupSpatialSigmaFactor", c_f),
        ("AlphaInterpolation", c_f),
    ]

    @classmethod
    def default(cls):
        return cls(0.025, 0.2, 0, 1, 0, 128, 0.3, 4.0, 1.0, 0.9, 0.9, 1.0)


class BloomAttribs(ctypes.Structure):
    _fields_ = [("Intensity", c_f), ("Threshold", c_f), ("SoftTreshold", c_f), ("Radius", c_f), ("AlphaInterpolation", c_f),
                ("Padding0", c_f), ("Padding1", c_f), ("Padding2", c_f)]

    @classmethod
    def default(cls):
        return cls(0.15, 1.0, 0.125, 0.75, 1.0, 0.0, 0.0, 0.0)


class DOFAttribs(ctypes.Structure):
    """DepthOfFieldAttribs -- Shaders/PostProcess/DepthOfField/public/DepthOfFieldStructures.fxh:31-56"""
    _fields_ = [("MaxCircleOfConfusion", c_f), ("TemporalStabilityFactor", c_f), ("BokehKernelRingCount", c_i), ("BokehKernelRingDensity", c_i),
                ("AlphaInterpolation", c_f), ("Padding0", c_f), ("Padding1", c_f), ("Padding2", c_f)]

    @classmethod
    def default(cls):
        return cls(0.01, 0.9375, 5, 7, 1.0, 0.0, 0.0, 0.0)


class TAAAttribs(ctypes.Structure):
    _fields_ = [("TemporalStabilityFactor", c_f), ("ResetAccumulation", c_i), ("SkipRejection", c_i), ("Padding0", c_f)]

    @classmethod
    def default(cls):
        return cls(0.9375, 0, 0, 0.0)


class PBRLightAttribs(ctypes.Structure):
    _fields_ = [
        ("Type", c_i), ("PosX", c_f), ("PosY", c_f), ("PosZ", c_f),
        ("DirectionX", c_f), ("DirectionY", c_f), ("DirectionZ", c_f), ("ShadowMapIndex", c_i),
        ("IntensityR", c_f), ("IntensityG", c_f), ("IntensityB", c_f), ("Range4", c_f),
        ("SpotAngleScale", c_f), ("SpotAngleOffset", c_f), ("Padding0", c_f), ("Padding1", c_f),
    ]


PBR_MAX_LIGHTS = 16


class PBRShadeAttribs(ctypes.Structure):
    _fields_ = [("IBLScale", c_f * 4), ("OcclusionStrength", c_f), ("EmissionScale", c_f), ("PrefilteredCubeLastMip", c_f),
                ("LightCount", c_i), ("Lights", PBRLightAttribs * PBR_MAX_LIGHTS), ("Workflow", c_i), ("Padding", c_i * 3)]


class PBRRendererShaderParameters(ctypes.Structure):  # PBR_Structures.fxh:126-149 (144 bytes)
    _fields_ = [("AverageLogLum", c_f), ("MiddleGray", c_f), ("WhitePoint", c_f), ("PrefilteredCubeLastMip", c_f), ("IBLScale", c_f * 4), ("OcclusionStrength", c_f),
                ("EmissionScale", c_f), ("PointSize", c_f), ("MipBias", c_f), ("LightCount", c_i), ("Time", c_f), ("DebugView", c_i), ("Padding0", c_f),
                ("UnshadedColor", c_f * 4), ("HighlightColor", c_f * 4), ("LoadingAnimation", c_f * 12)]


class PBRMaterialBasicAttribs(ctypes.Structure):  # PBR_Structures.fxh:154-180 (96 bytes)
    _fields_ = [("BaseColorFactor", c_f * 4), ("EmissiveFactor", c_f * 3), ("NormalScale", c_f), ("SpecularFactor", c_f * 3), ("ClearcoatNormalScale", c_f), ("Workflow", c_i),
                ("AlphaMode", c_i), ("AlphaMaskCutoff", c_f), ("MetallicFactor", c_f), ("RoughnessFactor", c_f), ("OcclusionFactor", c_f), ("ClearcoatFactor", c_f),
                ("ClearcoatRoughnessFactor", c_f), ("CustomData", c_f * 4)]


def pbr_frame_attribs(camera, prev_camera, renderer, lights, max_lights, shadow_maps=(), max_shadow_maps=0) -> bytes:
    """PBRFrameAttribs (RenderPBR_Structures.fxh:11-24) as the bytes of the renderer's frame constant buffer: Camera | PrevCamera | Renderer | Lights[max_lights] |
    ShadowMaps[max_shadow_maps]."""
    b = bytes(camera) + bytes(prev_camera) + bytes(renderer)
    b += b"".join(bytes(l) for l in lights) + bytes(64 * (max_lights - len(lights)))
    b += b"".join(bytes(s) for s in shadow_maps) + bytes(96 * (max_shadow_maps - len(shadow_maps)))
    return b


class DeviceDesc(ctypes.Structure):
    _fields_ = [("device", c_i), ("hip_stream", c_p)]


class PostFXCreateInfo(ctypes.Structure):
    _fields_ = [("sobol_256d", c_p), ("scrambling_tile", c_p)]


class FrameDesc(ctypes.Structure):
    _fields_ = [("Index", c_u), ("Width", c_u), ("Height", c_u), ("OutputWidth", c_u), ("OutputHeight", c_u)]


PImage = ctypes.POINTER(Image2D)


class PostFXRenderAttribs(ctypes.Structure):
    _fields_ = [("curr_depth", PImage), ("prev_depth", PImage), ("motion", PImage),
                ("curr_camera", ctypes.POINTER(CameraAttribs)), ("prev_camera", ctypes.POINTER(CameraAttribs))]


class SSAORenderAttribs(ctypes.Structure):
    _fields_ = [("postfx", c_p), ("depth", PImage), ("normal", PImage), ("attribs", ctypes.POINTER(SSAOAttribs))]


class SSRRenderAttribs(ctypes.Structure):
    _fields_ = [("postfx", c_p), ("color", PImage), ("depth", PImage), ("normal", PImage), ("material", PImage), ("motion", PImage),
                ("attribs", ctypes.POINTER(SSRAttribs))]


class TAARenderAttribs(ctypes.Structure):
    _fields_ = [("postfx", c_p), ("color", PImage), ("attribs", ctypes.POINTER(TAAAttribs))]


class BloomRenderAttribs(ctypes.Structure):
    _fields_ = [("postfx", c_p), ("color", PImage), ("attribs", ctypes.POINTER(BloomAttribs))]


class DOFRenderAttribs(ctypes.Structure):
    _fields_ = [("postfx", c_p), ("color", PImage), ("depth", PImage), ("attribs", ctypes.POINTER(DOFAttribs))]


class GBuffer(ctypes.Structure):
    _fields_ = [("base_color", PImage), ("normal", PImage), ("material", PImage), ("depth", PImage), ("emissive", PImage), ("occlusion", PImage)]


class IBL(ctypes.Structure):
    _fields_ = [("brdf_lut", PImage), ("irradiance", ctypes.POINTER(Cubemap)), ("prefiltered", ctypes.POINTER(Cubemap))]


PBR_LAYER_CLEAR_COAT, PBR_LAYER_SHEEN, PBR_LAYER_ANISOTROPY, PBR_LAYER_IRIDESCENCE, PBR_LAYER_TRANSMISSION = 1, 2, 4, 8, 16
PBR_LAYER_PLANES = ("clearcoat", "clearcoat_normal", "sheen", "anisotropy", "tangent", "iridescence", "transmission", "sheen_albedo_scaling_lut", "preintegrated_charlie")


class PBRLayers(ctypes.Structure):  # mifx_pbr_layers
    _fields_ = [("flags", c_u), ("iridescence_ior", c_f), ("anisotropy_rotation", c_f), ("padding", c_u)] + [(n, PImage) for n in PBR_LAYER_PLANES]


# PBR_Renderer::DebugViewType (PBR/interface/PBR_Renderer.hpp:401-439): PBR_DEBUG_VIEW_NONE = 0 ... PBR_DEBUG_VIEW_SCENE_DEPTH = 34
PBR_DEBUG_VIEWS = ("NONE", "TEXCOORD0", "TEXCOORD1", "BASE_COLOR", "TRANSPARENCY", "OCCLUSION", "EMISSIVE", "METALLIC", "ROUGHNESS", "DIFFUSE_COLOR", "SPECULAR_COLOR",
                   "REFLECTANCE90", "MESH_NORMAL", "SHADING_NORMAL", "MOTION_VECTORS", "NDOTV", "PUNCTUAL_LIGHTING", "DIFFUSE_IBL", "SPECULAR_IBL", "WHITE_BASE_COLOR", "CLEAR_COAT",
                   "CLEAR_COAT_FACTOR", "CLEAR_COAT_ROUGHNESS", "CLEAR_COAT_NORMAL", "SHEEN", "SHEEN_COLOR", "SHEEN_ROUGHNESS", "ANISOTROPY_STRENGTH", "ANISOTROPY_DIRECTION",
                   "IRIDESCENCE", "IRIDESCENCE_FACTOR", "IRIDESCENCE_THICKNESS", "TRANSMISSION", "THICKNESS", "SCENE_DEPTH")
for _i, _n in enumerate(PBR_DEBUG_VIEWS):
    globals()["PBR_DEBUG_VIEW_" + _n] = _i
PBR_DEBUG_VIEW_COUNT = len(PBR_DEBUG_VIEWS)
PBR_LOADING_ANIMATION_NONE, PBR_LOADING_ANIMATION_ALWAYS, PBR_LOADING_ANIMATION_TRANSITIONING = 0, 1, 2  # PBR_Renderer.hpp:441-447
PBR_ALPHA_MODE_OPAQUE, PBR_ALPHA_MODE_MASK, PBR_ALPHA_MODE_BLEND = 0, 1, 2  # PBR_Structures.fxh:34-44
PBR_SHADE_OUTPUT_FLAG_CONVERT_OUTPUT_TO_SRGB = 1
TONE_MAPPING_MODES = ("NONE", "EXP", "REINHARD", "REINHARD_MOD", "UNCHARTED2", "FILMIC_ALU", "LOGARITHMIC", "ADAPTIVE_LOG", "AGX", "AGX_CUSTOM", "PBR_NEUTRAL", "COMMERCE")


class PBRShadeOutputDesc(ctypes.Structure):  # mifx_pbr_shade_output_desc
    _fields_ = [("renderer", ctypes.POINTER(PBRRendererShaderParameters)), ("debug_view", c_i), ("tone_mapping_mode", c_i), ("loading_animation", c_i), ("alpha_mode", c_i),
                ("alpha_mask_cutoff", c_f), ("unlit", c_i), ("flags", c_u), ("padding", c_u), ("motion", PImage), ("mesh_normal", PImage)]


class PBRTargets(ctypes.Structure):  # mifx_pbr_targets: PSOut.Normal / BaseColor / Material / IBL of the USD footer (USD_Renderer.cpp:148-165)
    _fields_ = [("normal", PImage), ("base_color", PImage), ("material", PImage), ("ibl", PImage)]


class NativeImage(ctypes.Structure):  # mifx_native_image
    _fields_ = [("data", c_p), ("width", c_u), ("height", c_u), ("pitch_bytes", c_u), ("format", c_u)]


class GBufferNative(ctypes.Structure):  # mifx_gbuffer_native
    _P = ctypes.POINTER(NativeImage)
    _fields_ = [("base_color", _P), ("normal", _P), ("material", _P), ("depth", _P), ("emissive", _P), ("occlusion", _P)]


NATIVE_FORMATS = {name: i + 1 for i, name in enumerate(
    ["R32_FLOAT", "RG32_FLOAT", "RGBA32_FLOAT", "R16_FLOAT", "RG16_FLOAT", "RGBA16_FLOAT", "R8_UNORM", "RG8_UNORM", "RGBA8_UNORM", "RGBA8_UNORM_SRGB",
     "R16_UNORM", "RG16_UNORM", "RGBA16_UNORM", "R11G11B10_FLOAT"])}


class PBRShadowMapInfo(ctypes.Structure):
    """PBRShadowMapInfo -- Shaders/PBR/public/PBR_Structures.fxh:336-347 (96 bytes)"""
    _fields_ = [("WorldToLightProjSpace", c_f * 16), ("UVScale", c_f * 2), ("UVBias", c_f * 2), ("ShadowMapSlice", c_f), ("Padding0", c_f), ("Padding1", c_f), ("Padding2", c_f)]


class ShadowMapArray(ctypes.Structure):  # mifx_shadow_map_array
    _fields_ = [("data", c_p), ("width", c_u), ("height", c_u), ("slices", c_u), ("pitch_bytes", c_u), ("slice_pitch_bytes", ctypes.c_uint64)]


class PBRShadows(ctypes.Structure):  # mifx_pbr_shadows
    _fields_ = [("shadow_map", ctypes.POINTER(ShadowMapArray)), ("shadow_maps", ctypes.POINTER(PBRShadowMapInfo)), ("shadow_map_count", c_u), ("pcf_filter_size", c_u)]


class SphereMap(ctypes.Structure):  # mifx_spheremap
    _fields_ = [("mip_data", c_p * 16), ("width", c_u), ("height", c_u), ("mip_count", c_u)]


class EnvMapRenderAttribs(ctypes.Structure):
    """EnvMapRenderer::RenderAttribs -- Components/interface/EnvMapRenderer.hpp:97-118"""
    _fields_ = [("env_map", ctypes.POINTER(Cubemap)), ("average_log_lum", c_f), ("mip_level", c_f), ("alpha", c_f), ("options", c_u), ("scale", c_f * 3),
                ("sphere_map", ctypes.POINTER(SphereMap))]


class CompositeAttribs(ctypes.Structure):
    _fields_ = [("color", PImage), ("specular_ibl", PImage), ("ssr", PImage), ("ssao", PImage), ("normal", PImage), ("base_color", PImage),
                ("material", PImage), ("brdf_lut", PImage), ("camera", ctypes.POINTER(CameraAttribs)), ("ssr_scale", c_f), ("ssao_scale", c_f),
                ("tone_mapping", ctypes.POINTER(ToneMappingAttribs)), ("ave_log_lum", c_f)]


class SelectionAttribs(ctypes.Structure):
    """mifx_selection_attribs -- HnPostProcessTaskParams (HnPostProcessTask.hpp:79-85), HnProcessSelectionTaskParams::MaximumDistance (HnProcessSelectionTask.hpp:49)"""
    _fields_ = [("outline_color", c_f * 4), ("occluded_outline_color", c_f * 4), ("nonselection_desaturation", c_f), ("clear_depth", c_f),
                ("outline_width", c_f), ("max_distance", c_f), ("selection_id", ctypes.c_uint64)]

    @classmethod
    def default(cls, selection_id=0, clear_depth=1.0):
        return cls((c_f * 4)(1.0, 0.675, 0.25, 0.5), (c_f * 4)(0.375, 0.375, 0.125, 0.5), 0.0, clear_depth, 4.0, 4.0, selection_id)


class SelectionCompositeInputs(ctypes.Structure):  # mifx_selection_composite_inputs
    _fields_ = [("depth", PImage), ("selection_depth", PImage), ("closest_location", PImage), ("attribs", ctypes.POINTER(SelectionAttribs))]


class CoordinateGridAttribs(ctypes.Structure):
    """mifx_coordinate_grid_attribs -- CoordinateGridAttribs (Shaders/Common/public/CoordinateGridStructures.fxh:6-29), 192 bytes"""
    _fields_ = [("PositiveXAxisColor", c_f * 4), ("PositiveYAxisColor", c_f * 4), ("PositiveZAxisColor", c_f * 4), ("NegativeXAxisColor", c_f * 4),
                ("NegativeYAxisColor", c_f * 4), ("NegativeZAxisColor", c_f * 4), ("XAxisWidth", c_f), ("YAxisWidth", c_f), ("ZAxisWidth", c_f), ("Padding0", c_f),
                ("GridMajorColor", c_f * 4), ("GridMinorColor", c_f * 4), ("GridScale", c_f * 4), ("GridSubdivision", c_f * 4), ("GridLineWidth", c_f),
                ("GridMinCellWidth", c_f), ("GridMinCellSize", c_f), ("Padding1", c_f)]

    @classmethod
    def default(cls):
        """The reference's DEFAULT_VALUEs (what mifx_coordinate_grid_default_attribs writes)."""
        return cls((c_f * 4)(1, 0, 0, 1), (c_f * 4)(0, 1, 0, 1), (c_f * 4)(0, 0, 1, 1), (c_f * 4)(0.40, 0.15, 0.15, 1), (c_f * 4)(0.15, 0.40, 0.15, 1),
                   (c_f * 4)(0.15, 0.15, 0.40, 1), 3.0, 3.0, 3.0, 0.0, (c_f * 4)(0.4, 0.4, 0.4, 1), (c_f * 4)(0.1, 0.1, 0.1, 1), (c_f * 4)(1, 1, 1, 0),
                   (c_f * 4)(10, 10, 10, 0), 2.0, 4.0, 0.0001, 0.0)


# CoordinateGridRenderer::FEATURE_FLAGS (CoordinateGridRenderer.hpp:59-71)
COORDINATE_GRID_FEATURE_FLAG_NONE = 0
COORDINATE_GRID_FEATURE_FLAG_CONVERT_TO_SRGB = 1
COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_YZ = 2
COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XZ = 4
COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XY = 8
COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_X = 16
COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Y = 32
COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Z = 64
COORDINATE_GRID_DEBUG_FLAG_COORD = 256  # (not in the reference: the raw output holds Coord and fwidth(Coord))


MAX_CASCADES = 8
SHADOW_MODE_PCF, SHADOW_MODE_VSM, SHADOW_MODE_EVSM2, SHADOW_MODE_EVSM4 = 1, 2, 3, 4  # BasicStructures.fxh:19-22


class CascadeAttribs(ctypes.Structure):
    """mifx_cascade_attribs -- CascadeAttribs (Shaders/Common/public/BasicStructures.fxh:6-14), 64 bytes"""
    _fields_ = [("f4LightSpaceScale", c_f * 4), ("f4LightSpaceScaledBias", c_f * 4), ("f4StartEndZ", c_f * 4), ("f4MarginProjSpace", c_f * 4)]


class ShadowMapAttribs(ctypes.Structure):
    """mifx_shadow_map_attribs -- ShadowMapAttribs (BasicStructures.fxh:28-67), 1200 bytes"""
    _fields_ = [("mWorldToLightView", c_f * 16), ("Cascades", CascadeAttribs * MAX_CASCADES), ("mWorldToShadowMapUVDepth", (c_f * 16) * MAX_CASCADES),
                ("fCascadeCamSpaceZEnd", c_f * MAX_CASCADES), ("f4ShadowMapDim", c_f * 4), ("iNumCascades", c_i), ("fNumCascades", c_f), ("bVisualizeCascades", c_i),
                ("bVisualizeShadowing", c_i), ("fReceiverPlaneDepthBiasClamp", c_f), ("fFixedDepthBias", c_f), ("fCascadeTransitionRegion", c_f), ("iMaxAnisotropy", c_i),
                ("fVSMBias", c_f), ("fVSMLightBleedingReduction", c_f), ("fEVSMPositiveExponent", c_f), ("fEVSMNegativeExponent", c_f), ("bIs32BitEVSM", c_i),
                ("iFixedFilterSize", c_i), ("fFilterWorldSize", c_f), ("fDummy", c_i)]

    @classmethod
    def default(cls):
        """The reference's DEFAULT_VALUEs (what mifx_shadow_map_default_attribs writes); everything else is zero."""
        a = cls()
        a.fReceiverPlaneDepthBiasClamp, a.fFixedDepthBias, a.fCascadeTransitionRegion, a.iMaxAnisotropy = 10.0, 1e-5, 0.1, 4
        a.fVSMBias, a.fVSMLightBleedingReduction, a.fEVSMPositiveExponent, a.fEVSMNegativeExponent = 1e-4, 0.0, 40.0, 5.0
        a.bIs32BitEVSM, a.iFixedFilterSize, a.fFilterWorldSize = 1, 3, 0.0
        return a


class FilterableShadowMap(ctypes.Structure):  # mifx_filterable_shadow_map
    _fields_ = [("data", c_p), ("width", c_u), ("height", c_u), ("slices", c_u), ("format", c_u), ("pitch_bytes", c_u), ("slice_pitch_bytes", ctypes.c_uint64)]


class ShadowFilterParams(ctypes.Structure):  # mifx_shadow_filter_params: the compile-time macros of Shadows.fxh
    _fields_ = [("shadow_mode", c_u), ("filter_across_cascades", c_u), ("best_cascade_search", c_u), ("reserved", c_u)]


def shadow_map_array(t) -> "ShadowMapArray":
    """float32 CUDA tensor (slices, H, W), rows and slices possibly pitched -> mifx_shadow_map_array"""
    assert t.dim() == 3 and t.stride(2) == 1, "a (slices, H, W) float32 tensor with contiguous texels"
    return ShadowMapArray(t.data_ptr(), t.shape[2], t.shape[1], t.shape[0], t.stride(1) * 4, t.stride(0) * 4)


def filterable_shadow_map(t) -> FilterableShadowMap:
    """CUDA tensor (slices, H, W, 2 | 4), rows and slices possibly pitched -> mifx_filterable_shadow_map.  float32: F32X2 / F32X4; the 16-bit filterable formats:
    float16 (…, 2) = F16X2 (RG16_FLOAT), float16 (…, 4) = F16X4 (RGBA16_FLOAT), int16 (…, 2) = U16X2 (the codes of RG16_UNORM)"""
    assert t.dim() == 4 and t.shape[3] in (2, 4) and t.stride(3) == 1 and t.stride(2) == t.shape[3], "a (slices, H, W, 2 | 4) tensor with contiguous texels"
    import torch

    fmt = {(torch.float32, 2): FORMAT_F32X2, (torch.float32, 4): FORMAT_F32X4, (torch.float16, 2): FORMAT_F16X2, (torch.float16, 4): FORMAT_F16X4,
           (torch.int16, 2): FORMAT_U16X2}.get((t.dtype, t.shape[3]))
    assert fmt is not None, f"no filterable shadow-map format for {t.dtype} x {t.shape[3]}"
    return FilterableShadowMap(t.data_ptr(), t.shape[2], t.shape[1], t.shape[0], fmt, t.stride(1) * t.element_size(), t.stride(0) * t.element_size())


OIT_MAX_SLICES, OIT_MAX_LAYERS = 32, 16  # MIFX_OIT_MAX_SLICES, MIFX_OIT_MAX_LAYERS


class OITSlice(ctypes.Structure):  # mifx_oit_slice: one transparent draw
    _fields_ = [("depth", PImage), ("base_color", PImage), ("material", PImage), ("radiance", PImage), ("specular_ibl", PImage), ("color_alpha", PImage)]


class OITTargets(ctypes.Structure):  # mifx_oit_targets: blended in place
    _fields_ = [("color", PImage), ("base_color", PImage), ("material", PImage), ("ibl", PImage)]


class TransparentSlice(ctypes.Structure):  # mifx_transparent_slice: one transparent draw as its own G-buffer (mifx_oit_shade_blend, mifx_chain_set_transparency)
    _fields_ = [("gbuffer", GBuffer), ("layers", ctypes.POINTER(PBRLayers)), ("color_alpha", PImage)]


class ChainFrame(ctypes.Structure):
    _fields_ = [("frame", FrameDesc), ("gbuffer", GBuffer), ("motion", PImage), ("prev_depth", PImage),
                ("curr_camera", ctypes.POINTER(CameraAttribs)), ("prev_camera", ctypes.POINTER(CameraAttribs)),
                ("ibl", ctypes.POINTER(IBL)), ("pbr", ctypes.POINTER(PBRShadeAttribs)), ("ssao", ctypes.POINTER(SSAOAttribs)),
                ("ssr", ctypes.POINTER(SSRAttribs)), ("taa", ctypes.POINTER(TAAAttribs)), ("bloom", ctypes.POINTER(BloomAttribs)),
                ("tone_mapping", ctypes.POINTER(ToneMappingAttribs)), ("ave_log_lum", c_f), ("ssr_scale", c_f), ("ssao_scale", c_f),
                ("background", c_f * 4), ("taa_feature_flags", c_u), ("tonemap_flags", c_u)]


SIZEOF_NAMES = {
    "image2d": Image2D, "cubemap": Cubemap, "camera_attribs": CameraAttribs, "tone_mapping_attribs": ToneMappingAttribs,
    "ssao_attribs": SSAOAttribs, "ssr_attribs": SSRAttribs, "bloom_attribs": BloomAttribs, "dof_attribs": DOFAttribs, "taa_attribs": TAAAttribs,
    "pbr_light_attribs": PBRLightAttribs, "pbr_shade_attribs": PBRShadeAttribs, "frame_desc": FrameDesc, "chain_frame": ChainFrame,
    "composite_attribs": CompositeAttribs, "gbuffer": GBuffer, "ibl": IBL, "pbr_shadow_map_info": PBRShadowMapInfo,
    "selection_attribs": SelectionAttribs, "selection_composite_inputs": SelectionCompositeInputs, "coordinate_grid_attribs": CoordinateGridAttribs,
    "cascade_attribs": CascadeAttribs, "shadow_map_attribs": ShadowMapAttribs, "filterable_shadow_map": FilterableShadowMap, "shadow_filter_params": ShadowFilterParams,
}

_lib = None


def load():
    """Loads libmifx.so; raises (loudly) when it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python diligentfx_amd/build.py` (hipcc, gfx950). "
                              "diligentfx_amd has no CPU or PyTorch fallback.")
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.mifx_status_string.restype = ctypes.c_char_p
        _lib.mifx_last_error.restype = ctypes.c_char_p
        _lib.mifx_sizeof.restype = c_u
        _lib.mifx_sizeof.argtypes = [ctypes.c_char_p]
        _lib.mifx_abi_version.restype = c_u
        _lib.mifx_storage_mode.restype = c_u
        assert bool(_lib.mifx_storage_mode()) == STORAGE_H4 or os.environ.get("MIFX_LIB_PATH"), "the loaded library is not the storage build MIFX_STORAGE asks for"
        _declare_oit(_lib)
        if hasattr(_lib, "mifx_pbr_material_fetch"):  # (a library named by MIFX_LIB_PATH may be built from the host sources alone: the entries live beside their kernel)
            declare_material_fetch(_lib)
    return _lib


def _declare_oit(lib):
    """Prototypes of the order-independent-transparency entries (include/mifx.h)"""
    PS, PT, PC, u = ctypes.POINTER(OITSlice), ctypes.POINTER(OITTargets), ctypes.POINTER(CameraAttribs), c_u
    lib.mifx_oit_create.argtypes = [c_p, u, u, u, ctypes.POINTER(c_p)]
    lib.mifx_oit_destroy.argtypes, lib.mifx_oit_destroy.restype = [c_p], None
    lib.mifx_oit_clear_layers.argtypes = [c_p]
    lib.mifx_oit_update_layers.argtypes = [c_p, PS, PImage, PC]
    lib.mifx_oit_apply_attenuation.argtypes = [c_p, PT]
    lib.mifx_oit_blend.argtypes = [c_p, PS, PImage, PC, PT]
    lib.mifx_oit_build_layers.argtypes = [c_p, PS, u, PImage, PC]
    lib.mifx_oit_resolve.argtypes = [c_p, PS, u, PImage, PC, PT]
    lib.mifx_oit_get_layers.argtypes = [c_p, ctypes.POINTER(c_p), ctypes.POINTER(ctypes.c_uint64)]
    lib.mifx_oit_get_tail.argtypes = [c_p, PImage]
    lib.mifx_oit_set_fusion.argtypes, lib.mifx_oit_set_fusion.restype = [c_i], c_i
    lib.mifx_oit_create_check.argtypes = [u, u, u]
    lib.mifx_oit_frame_check.argtypes = [u, u, PS, u, PImage, PC, PT]
    PX, PA, PI, PH = ctypes.POINTER(TransparentSlice), ctypes.POINTER(PBRShadeAttribs), ctypes.POINTER(IBL), ctypes.POINTER(PBRShadows)
    lib.mifx_oit_shade_blend.argtypes = [c_p, PX, PImage, PC, PA, PI, PH, PT]
    lib.mifx_oit_shade_blend_check.argtypes = [u, u, u, PX, PImage, PC, PA, PI, PH, PT]
    lib.mifx_chain_set_transparency.argtypes, lib.mifx_chain_set_transparency.restype = [c_p, u, PX, u], c_i
    lib.mifx_chain_set_transparency_fusion.argtypes, lib.mifx_chain_set_transparency_fusion.restype = [c_i], c_i
    for name in ("create", "clear_layers", "update_layers", "apply_attenuation", "blend", "build_layers", "resolve", "get_layers", "get_tail", "create_check", "frame_check",
                 "shade_blend", "shade_blend_check"):
        getattr(lib, "mifx_oit_" + name).restype = c_i


def device_code_sha16(path=None):
    """Identity of the DEVICE code of a library build: the first 16 hex digits of the SHA-256 of its `.hip_fatbin` section (the gfx950 code objects hipcc embeds; host-side
    changes -- api_*.cpp -- leave it alone).  What ties a committed counter file to the kernels a run times: tools/pmc_traffic.py stamps it into profiles/rNN_pmc_traffic.json,
    bench.py compares it with the library it has loaded (roofline.traffic_matches_build).  None when the file has no such section."""
    import hashlib
    import struct

    path = path or LIB_PATH
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        return None
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    sec = lambda i: struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize)  # noqa: E731  name, type, flags, addr, offset, size, link, info, align, entsize
    stroff = sec(shstrndx)[4]
    for i in range(shnum):
        name_off, _, _, _, off, size = sec(i)[:6]
        end = data.index(b"\0", stroff + name_off)
        if data[stroff + name_off:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()[:16]
    return None


def storage_dtype():
    """torch dtype of a 4-channel image in this process: float32, or float16 with MIFX_STORAGE=h4 (1- and 2-channel images are float32 in both)."""
    import torch

    return torch.float16 if load().mifx_storage_mode() == 1 else torch.float32


def plane_dtype(kind):
    """torch dtype of an effect-owned plane of the loaded library: kind "colour" (4 channels), "ao" / "roughness" (R8_UNORM in the native-storage build),
    "history_len" / "variance" (R16_FLOAT), "motion" (closest motion, RG16_FLOAT); float32 throughout in the fp32 build."""
    import torch

    if storage_dtype() == torch.float32:
        return torch.float32
    return {"colour": torch.float16, "ao": torch.uint8, "roughness": torch.uint8, "history_len": torch.float16, "variance": torch.float16, "motion": torch.float16}[kind]


def to_storage(t):
    """A float32 (H, W, 4) tensor as the 4-channel image of this process' storage mode (rounded to nearest-even binary16 with MIFX_STORAGE=h4)."""
    return t.to(storage_dtype()).contiguous() if t.dim() == 3 and t.shape[2] == 4 else t


class ShardInfo(ctypes.Structure):  # mifx_shard_info
    _fields_ = [("band_begin", ctypes.c_int32), ("band_end", ctypes.c_int32), ("halo_taa", ctypes.c_int32), ("halo_ssr", ctypes.c_int32),
                ("halo_ssao", ctypes.c_int32), ("gather_level", ctypes.c_int32), ("own_begin", ctypes.c_int32), ("own_end", ctypes.c_int32),
                ("ae_begin", ctypes.c_int32), ("ae_end", ctypes.c_int32)]


class CommStats(ctypes.Structure):  # mifx_comm_stats
    _fields_ = [("rank", ctypes.c_int32), ("world", ctypes.c_int32), ("is_rccl", ctypes.c_int32), ("ranks_in_communicator", ctypes.c_int32),
                ("groups", ctypes.c_uint64), ("bytes_sent", ctypes.c_uint64), ("bytes_received", ctypes.c_uint64),
                ("timed_groups", ctypes.c_uint32), ("exchange_ms_total", ctypes.c_float), ("exchange_ms_max", ctypes.c_float)]


SIZEOF_NAMES.update({"pbr_shade_output_desc": PBRShadeOutputDesc, "pbr_targets": PBRTargets, "shard_info": ShardInfo, "comm_stats": CommStats, "oit_slice": OITSlice, "oit_targets": OITTargets})


# ---- the material fetch (include/mifx.h "material fetch")
PBR_TEXTURE_SLOTS = ("BASE_COLOR", "PHYS_DESC", "NORMAL", "OCCLUSION", "EMISSIVE", "METALLIC", "ROUGHNESS", "CLEAR_COAT", "CLEAR_COAT_ROUGHNESS", "CLEAR_COAT_NORMAL", "SHEEN_COLOR",
                     "SHEEN_ROUGHNESS", "ANISOTROPY", "IRIDESCENCE", "IRIDESCENCE_THICKNESS", "TRANSMISSION")
for _i, _n in enumerate(PBR_TEXTURE_SLOTS):
    globals()["PBR_TEXTURE_" + _n] = _i
PBR_TEXTURE_COUNT = len(PBR_TEXTURE_SLOTS)
MATERIAL_FETCH_FLAG_TEXTURE_ATLAS, MATERIAL_FETCH_FLAG_TEXCOORD_TRANSFORM, MATERIAL_FETCH_FLAG_SRGB_TO_LINEAR = 1, 2, 4
TEXTURE_ADDRESS_WRAP, TEXTURE_ADDRESS_CLAMP = 1, 3


class TextureArray(ctypes.Structure):  # mifx_texture_array
    _fields_ = [("data", c_p), ("width", c_u), ("height", c_u), ("slices", c_u), ("mips", c_u), ("format", c_u), ("padding", c_u), ("slice_pitch_bytes", ctypes.c_uint64)]


class PBRTextureAttribs(ctypes.Structure):  # PBRMaterialTextureAttribs, PBR_Structures.fxh:245-254 (48 bytes)
    _fields_ = [("PackedProps", c_u), ("TextureSlice", c_f), ("UBias", c_f), ("VBias", c_f), ("UVScaleAndRotation", c_f * 4), ("AtlasUVScaleAndBias", c_f * 4)]

    @classmethod
    def make(cls, uv_selector=0, wrap_u=TEXTURE_ADDRESS_WRAP, wrap_v=TEXTURE_ADDRESS_WRAP, slice=0.0, bias=(0.0, 0.0), scale_rotation=(1.0, 0.0, 0.0, 1.0),
             atlas=(1.0, 1.0, 0.0, 0.0)):
        """GLTF::Material::TextureShaderAttribs: selector -1 = none, 0 = UV0, 1 = UV1; wrap modes are TEXTURE_ADDRESS_* values"""
        packed = ((uv_selector + 1) & 7) | (((wrap_u - 1) & 7) << 3) | (((wrap_v - 1) & 7) << 6)
        return cls(packed, slice, bias[0], bias[1], (c_f * 4)(*scale_rotation), (c_f * 4)(*atlas))


class PBRMaterial(ctypes.Structure):  # mifx_pbr_material (1008 bytes)
    _fields_ = [("basic", PBRMaterialBasicAttribs), ("sheen", c_f * 4), ("anisotropy", c_f * 4), ("iridescence", c_f * 4), ("transmission", c_f * 4), ("fallback_color", c_f * 4),
                ("textures", PBRTextureAttribs * PBR_TEXTURE_COUNT), ("texture", c_i * PBR_TEXTURE_COUNT)]


class MaterialInterpolants(ctypes.Structure):  # mifx_material_interpolants
    _fields_ = [(n, PImage) for n in ("depth", "uv0", "uv1", "mesh_normal", "color", "face", "material_index")]


class MaterialFetchDesc(ctypes.Structure):  # mifx_material_fetch_desc
    _fields_ = [("materials", ctypes.POINTER(PBRMaterial)), ("textures", ctypes.POINTER(TextureArray)), ("material_count", c_u), ("texture_count", c_u), ("layer_flags", c_u),
                ("flags", c_u), ("mip_bias", c_f), ("padding", c_u * 3)]


SIZEOF_NAMES.update({"texture_array": TextureArray, "pbr_texture_attribs": PBRTextureAttribs, "pbr_material": PBRMaterial, "material_interpolants": MaterialInterpolants,
                     "material_fetch_desc": MaterialFetchDesc})


def declare_material_fetch(lib):
    """Prototypes of the two material-fetch entries (any build of the library)"""
    PM, PD, PC, PG, PL = ctypes.POINTER(MaterialInterpolants), ctypes.POINTER(MaterialFetchDesc), ctypes.POINTER(CameraAttribs), ctypes.POINTER(GBuffer), ctypes.POINTER(PBRLayers)
    lib.mifx_pbr_material_fetch_check.argtypes, lib.mifx_pbr_material_fetch_check.restype = [PM, PD, PC, PG, PL], c_i
    lib.mifx_pbr_material_fetch.argtypes, lib.mifx_pbr_material_fetch.restype = [c_p, PM, PD, PC, PG, PL], c_i
    return lib


class MifxError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__(f"{status}: {detail}")
        self.status = status


def check(status):
    if status < 0:
        lib = load()
        raise MifxError(lib.mifx_status_string(status).decode(), lib.mifx_last_error().decode())
    return status


def image(t) -> Image2D:
    """torch CUDA float32 tensor (H,W) / (H,W,2) / (H,W,4), or float16 (H,W,4) (MIFX_FORMAT_F16X4, the RGBA16_FLOAT storage build), row-contiguous -> mifx_image2d."""
    import torch

    assert isinstance(t, torch.Tensor) and t.dtype in (torch.float32, torch.float16, torch.uint8, torch.int32), "images are float32 tensors (native-storage build: also float16 / uint8 / packed int32)"
    if t.dim() == 2:
        c = 1
    else:
        assert t.dim() == 3 and t.shape[2] in (2, 4), t.shape
        c = t.shape[2]
    assert t.stride(-1) == 1 and (t.dim() == 2 or t.stride(1) == c), "texels must be contiguous"
    if t.dtype == torch.uint8:   # R8_UNORM (ambient occlusion, SSR roughness)
        assert c == 1
        return Image2D(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0), FORMAT_U8)
    if t.dtype == torch.int32:   # R11G11B10_FLOAT, one packed texel per element (Bloom levels)
        assert c == 1
        return Image2D(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * 4, FORMAT_R11G11B10)
    if t.dtype == torch.float16:
        return Image2D(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * 2, {1: FORMAT_F16, 2: FORMAT_F16X2, 4: FORMAT_F16X4}[c])
    pitch = t.stride(0) * 4
    return Image2D(t.data_ptr(), t.shape[1], t.shape[0], pitch, {1: FORMAT_F32, 2: FORMAT_F32X2, 4: FORMAT_F32X4}[c])


def camera_from_bytes(b: bytes) -> CameraAttribs:
    assert len(b) == ctypes.sizeof(CameraAttribs)
    return CameraAttribs.from_buffer_copy(b)


def as_bytes(struct) -> bytes:
    return bytes(struct)
