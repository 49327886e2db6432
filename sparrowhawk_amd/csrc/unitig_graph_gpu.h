// unitig_graph_gpu.h — the device twin of unitig_assemble (unitig_graph.h): SPEC S9 and S10 on unitig records as HIP kernels.
// The index of chain starts, the links (mirror strands, out-neighbours), the tip and bubble rounds, the simple successors
// and the walk of the chains (heads, ranks by pointer jumping, strand choice, placement) run on the current GPU.  The
// linear contigs come back in the flat form of UnitigGraphResult (flat, lin, recs_flat, place): the same contigs in the same
// order as unitig_chains appends them, with the text offsets and node offsets the layout of the sharded assembly needs;
// the ring records come back as a list and go through the host's ring loops (unitig_ring_chains) into out.contigs.
// With SHK_UNITIG_CHAINS_DEVICE=0 alive / mirror / succ come back instead and unitig_chains (the host's own S10 walk)
// builds out.contigs from them, field by field what unitig_assemble builds.
#pragma once
#include "unitig_graph.h"

namespace shk {

// 0: out filled — contigs, need_min, removal counts and rounds as unitig_assemble fills them, the linear contigs in the
//    flat form when the walk ran here (out.flat);
// -1: inconsistent input, err = the host's message, word for word;
// 1: not run (out of device memory, nothing is held) — the caller runs the host code;
// -5: HIP error
int unitig_assemble_device(int k, const std::vector<UnitigRec> &recs, bool tips, bool bubbles, int device, void *stream,
                           UnitigGraphResult &out, std::string &err);

// The S10 walk alone on the device, from settled arrays: the twin of unitig_chains.  The arrays must pass
// unitig_chains_check.  Always the flat form; same return values.
int unitig_chains_device(int k, const std::vector<UnitigRec> &recs, const std::vector<uint8_t> &alive, const std::vector<uint32_t> &mirror,
                         const std::vector<uint32_t> &succ, int device, void *stream, UnitigGraphResult &out, std::string &err);

}  // namespace shk
