"""Worker of tests/test_gpu_shard_fasta.py (launched with torch.distributed.run): shk_shard_preprocess_fasta and the collective
shk_assemble over the library's own communicator.  torch.distributed (gloo) only carries the ncclUniqueId; rank r uses
cuda:(r % device_count).  One launch runs a list of cases on one communicator:

    cfg["cases"] = [{"files": [[file1, file2 | null] | null, ...  one entry per rank], "split": 0 | 1, "k", "min_count",
                     "env": {name: value} (optional: set on every rank for this case)}]

Every rank writes the list of its results, {"pre", "asm", "timings"} or {"error", "code"}, to <out>.<rank>."""
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
    from sparrowhawk_amd.dist import LibComm, sharded_preprocess_fasta
    torch.cuda.set_device(torch.device("cuda", rank % max(1, torch.cuda.device_count())))
    cfg = json.load(open(cfg_path))
    comm = LibComm(rank, world)
    results = []
    for cs in cfg["cases"]:
        mine = cs["files"][rank] or [None, None]
        f1, f2 = (open(p, "rb").read() if p else None for p in mine)
        env = cs.get("env", {})
        for name, value in env.items():
            os.environ[name] = str(value)
        h = AssemblyHelper.new(cs["k"], True, cs["min_count"], 20, 0, False, False, False, False)
        try:
            sharded_preprocess_fasta(h, comm, f1, f2, split=bool(cs["split"]))
            h.assemble()
            res = {"pre": h.get_preprocessing_info(), "asm": h.get_assembly(), "timings": h.timings()}
        except ShkError as e:
            # every rank gets here together (the error agreement inside the call): none may hang
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
