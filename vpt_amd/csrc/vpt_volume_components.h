// vpt_volume_components.h — the object behind a vpt_components handle, for the two units that work on it: vpt_volume_components.hip builds
// it (labelling, list, ranks) and vpt_volume_measure.hip reads it (per-component measurements, selection by a set of ranks).
#pragma once
#include "vpt_volume_field.h"

struct vpt_components : VoxelField {       // the values are L: at the end one rank per voxel
    std::vector<vpt_component> list;        // canonical order
    struct vpt_components_info info = {};
    double ms[VPT_COMPONENTS_PHASES] = {};
    uint32_t launches[2] = {};
};
