"""Worker of tests/test_gpu_bgzf_write.py (launched with torch.distributed.run): a sharded assembly from one FASTQ file over the
library's own communicator, then shk_get_assembly_bgzf on every rank.  torch.distributed (gloo) only carries the
ncclUniqueId; rank r uses cuda:(r % device_count).

    cfg = {"fastq": path, "k": k, "runs": [{"env": {name: value}, "request": mask | null}, ...]}

Every rank writes the list of its results, {"asm", "files": [hex x 4], "timings"} or {"error", "code"}, to <out>.<rank>."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_path, cfg_path = sys.argv[1], sys.argv[2]
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from sparrowhawk_amd import AssemblyHelper, ShkError
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fastq
    torch.cuda.set_device(torch.device("cuda", rank % max(1, torch.cuda.device_count())))
    cfg = json.load(open(cfg_path))
    fq = open(cfg["fastq"], "rb").read()
    comm = LibComm(rank, world)
    results = []
    for run in cfg["runs"]:
        env = run.get("env", {})
        for name, value in env.items():
            os.environ[name] = str(value)
        h = AssemblyHelper.new(cfg["k"], True, 0, 0, 0, False, False, True, True)
        try:
            if run.get("request") is not None:
                h.request_assembly_bgzf(run["request"])
            sharded_preprocess_fastq(h, comm, fq, split=True)
            h.assemble()
            res = {"asm": h.get_assembly(), "files": [h.get_assembly_bgzf(w).hex() for w in range(4)], "timings": h.timings()}
        except ShkError as e:
            res = {"error": str(e), "code": e.code}
        for name in env:
            os.environ.pop(name, None)
        results.append(res)
        h.free()
    with open(f"{out_path}.{rank}", "w") as f:
        json.dump(results, f)
    comm.free()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
