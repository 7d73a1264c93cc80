"""Write tests/golden/str_hash.json: std::hash<std::string> of a fixed set of keys, as g++'s libstdc++ computes it on a
64-bit target (_Hash_bytes, seed 0xc70f6907) -- the hash the reference orders string keys by (radix_hash.h:86-109) and
hmj_hash_str_device restates.  A few-line C++ program reads the keys as hex, one per line, and prints their hashes;
only the data is committed.

Keys: every length 0..80 (bytes (7 * i + 3 * len) mod 256, so high bytes and NUL occur), strings with NUL and high
bytes, UTF-8 text, 300 words of tests/golden/words.txt and 300 strgen "a-b" keys built from them.
Run: python3 tests/golden/make_str_hash.py   (needs g++)"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

PROG = r"""
#include <functional>
#include <iostream>
#include <string>
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::string key;
    for (size_t i = 0; i + 1 < line.size(); i += 2) key.push_back((char)std::stoi(line.substr(i, 2), nullptr, 16));
    std::cout << std::hash<std::string>()(key) << "\n";
  }
}
"""


def keys():
    out = [bytes((7 * i + 3 * n) & 0xFF for i in range(n)) for n in range(81)]
    out += [b"\x00", b"\x00\x00", b"a\x00b", b"\x00" * 9, b"\xff", b"\xff" * 8, b"\x80\x81\x82\x83\x84\x85\x86",
            b"abc\x00def\x00ghi", bytes(range(256)), "héllo wörld".encode(), "日本語のキー".encode(), b"A" * 1000]
    words = open(os.path.join(HERE, "words.txt")).read().split("\n")
    words = [w for w in words if w][:300]
    out += [w.encode() for w in words]
    out += [(words[i % 300] + "-" + words[(7 * i + 3) % 300]).encode() for i in range(300)]
    return out


def main():
    ks = keys()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "h.cc"), os.path.join(d, "h")
        open(src, "w").write(PROG)
        subprocess.check_call(["g++", "-O1", "-std=c++11", src, "-o", exe])
        txt = subprocess.run([exe], input="".join(k.hex() + "\n" for k in ks).encode(), stdout=subprocess.PIPE,
                             check=True).stdout.decode()
    hs = [int(x) for x in txt.split()]
    assert len(hs) == len(ks)
    doc = {"_about": "std::hash<std::string> (libstdc++, 64-bit) of each key; keys as hex. tests/golden/make_str_hash.py",
           "cases": [{"key_hex": k.hex(), "hash": h} for k, h in zip(ks, hs)]}
    with open(os.path.join(HERE, "str_hash.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote %d hashes" % len(hs))


if __name__ == "__main__":
    main()
