"""Writes tests/golden/zstd_streams.json: libzstd's streams (base64) of the inputs tests/zstd_frames.golden_inputs() generates --
levels -5, 1, 3 and 19, checksum and content-size flags on and off, one stream written with flushes.  Needs libzstd.
Run from the repository root: python tests/golden/make_zstd_golden.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import zstd_frames as zf  # noqa: E402

if __name__ == "__main__":
    with open(zf.GOLDEN, "w") as f:
        json.dump(zf.make_golden(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(os.path.getsize(zf.GOLDEN), "bytes")
