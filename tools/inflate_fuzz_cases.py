"""Write the valid zlib streams of tests/inflate_cases.py as input files for tools/inflate_fuzz.cpp:
one file per stream, a little-endian u64 with the inflated length, then the stream.

Usage: python tools/inflate_fuzz_cases.py DIR      (prints the files' paths, one per line)
"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import inflate_cases

    folder = sys.argv[1]
    os.makedirs(folder, exist_ok=True)
    for name, stream, payload in inflate_cases.valid_cases():
        path = os.path.join(folder, name + ".bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(payload)) + stream)
        print(path)


if __name__ == "__main__":
    main()
