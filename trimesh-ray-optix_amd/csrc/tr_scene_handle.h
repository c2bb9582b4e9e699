// tr_scene_handle.h -- INTERNAL: the opaque tr_scene of include/triro_scene.h and its stale check, shared by the libraries
// that read a committed scene (scene.hip, which owns the handle: create, commit, destroy; scene_cross.hip, which only reads
// it).  Host only.  Not installed: nothing outside csrc/ includes it.
#pragma once
#include <vector>

#include "tr_internal.h"
#include "tr_scene.h"

// the opaque handle ---------------------------------------------------------------------
struct tr_scene {
    int device = 0;
    void* table = nullptr;          // one hipMalloc: members | instances (grown only)
    size_t table_bytes = 0;
    std::vector<const tr_bvh*> members;          // the handles, as given to the last commit
    std::vector<tr_scene_member> committed;      // ... and their arrays and counts as they were then (the stale check)
    int64_t ninst = 0, nvalid = 0, commits = 0;
    const tr_scene_member* d_members = nullptr;
    const tr_scene_inst* d_insts = nullptr;
};

// has any member's arrays, count or device changed since the commit?  (host only: reads the handles)
static inline bool scene_stale(const tr_scene* s) {
    for (size_t k = 0; k < s->members.size(); k++) {
        const tr_bvh* b = s->members[k];
        const tr_scene_member& c = s->committed[k];
        if (b->device != s->device || b->nodes != c.nodes || b->links != c.links || b->tris != c.tris || b->num_tris != c.num_tris)
            return true;
    }
    return false;
}
