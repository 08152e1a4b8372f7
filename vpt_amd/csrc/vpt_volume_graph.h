// vpt_volume_graph.h — the handle behind vpt_graph (vpt_volume_graph.hip): the two labellings of a voxel set's classes (branches, nodes), the
// class field they were made from, and the records the links pass and the host made of them.
#pragma once
#include "vpt_volume_components.h"
#include "vpt_volume_skeleton.h"

struct vpt_graph {
    vpt_context *ctx = nullptr;
    std::unique_ptr<vpt_components> branches, nodes;      // the graph's own; the C-ABI hands out copies (both hold the source's codes as texels)
    DevBuf<uint8_t> classes;                              // one byte per voxel, in the texels' linear order
    std::vector<vpt_graph_branch> branch;                 // canonical order
    std::vector<vpt_graph_node> node;
    struct vpt_graph_info info = {};
    double ms[VPT_GRAPH_PHASES] = {};
    uint64_t launches = 0;
};
