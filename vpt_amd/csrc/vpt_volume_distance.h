// vpt_volume_distance.h — the handle behind vpt_distance and what the distance unit (vpt_volume_distance.hip) offers the unit that builds
// such a handle from another one (vpt_volume_thickness.hip: the values are squared local thicknesses).
#pragma once
#include "vpt_volume_field.h"

#define EDT_NONE 0xFFFFFFFFu

struct vpt_distance : VoxelField {         // the values are d2: one squared distance per voxel
    struct vpt_distance_info info = {};
    double ms[VPT_DISTANCE_PHASES] = {};
};

// enqueues k_largest on `st`: atomicMax of the finite values of d2[0 .. n) into *largest (a device word the caller has zeroed)
int distance_largest(hipStream_t st, const uint32_t *d2, size_t n, uint32_t *largest);
