// vpt_volume_skeleton.h — the handle behind vpt_skeleton (vpt_volume_skeleton.hip): a voxel field whose values are burn passes.
#pragma once
#include "vpt_volume_field.h"

struct vpt_skeleton : VoxelField {         // the values are burn passes: 0 outside the range, k deleted in pass k, VPT_THIN_KEPT survived
    struct vpt_skeleton_info info = {};
    double ms[VPT_SKELETON_PHASES] = {};
    uint64_t launches = 0, tile_visits = 0;
};
