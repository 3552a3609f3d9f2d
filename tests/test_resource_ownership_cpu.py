"""CPU-side check (no GPU): the host layer's device memory, pinned memory, events and streams are held by the owning
types of csrc/ctx.hpp (DevBuf, HostBuf, Event, Stream), so the HIP functions that make or release them are named in that
header and nowhere else under csrc/.  A new buffer is a new member of an owning type, not a new allocate / free pair."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximategps.jl_amd", "csrc")
RAW = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipEventCreate\w*|hipEventDestroy|hipStreamCreate\w*|hipStreamDestroy)\b")


def test_raw_resource_calls_live_in_ctx_hpp_only():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    assert any(f.endswith("api.hip") for f in files) and any(f.endswith("ctx.hpp") for f in files)
    hits = []
    for f in files:
        if os.path.basename(f) == "ctx.hpp":
            continue
        for no, line in enumerate(open(f), 1):   # comments and strings count: a reader greps for these names
            if RAW.search(line):
                hits.append(f"{os.path.basename(f)}:{no}: {line.strip()[:100]}")
    assert not hits, f"{len(hits)} raw resource calls outside ctx.hpp:\n" + "\n".join(hits[:20])
    # the header does hold them (a rename of the HIP functions would otherwise make this test pass vacuously)
    assert len(RAW.findall(open(os.path.join(CSRC, "ctx.hpp")).read())) >= 8
