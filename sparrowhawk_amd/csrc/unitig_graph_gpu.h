// unitig_graph_gpu.h — the device twin of unitig_assemble (unitig_graph.h): SPEC S9 on unitig records as HIP kernels.
// The index of chain starts, the links (mirror strands, out-neighbours), the tip and bubble rounds and the simple
// successors run on the current GPU; alive / mirror / succ come back and unitig_chains (the host's own S10 walk) builds
// the contigs from them.  Same records in, same UnitigGraphResult out, field by field.
#pragma once
#include "unitig_graph.h"

namespace shk {

// 0: out filled exactly as unitig_assemble fills it;
// -1: inconsistent input, err = the host's message, word for word;
// 1: not run (out of device memory) — the caller runs the host code;
// -5: HIP error
int unitig_assemble_device(int k, const std::vector<UnitigRec> &recs, bool tips, bool bubbles, int device, void *stream,
                           UnitigGraphResult &out, std::string &err);

}  // namespace shk
