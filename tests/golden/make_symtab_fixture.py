#!/usr/bin/env python3
"""The word list of the wordloop graph, in the reference's symbol-table file format.

    python3 tests/golden/make_symtab_fixture.py     ->  tests/golden/refmodel/wordloop_words.bin

OUR names (nothing of the reference's data), written in the layout pk_symboltable_read parses
(symbol_table.cc:23-73): "SYM0", i32 section size (= 8 + 4 size + buffer_size), i32 size, i32
buffer_size, size x i32 offsets into the buffer, then buffer_size bytes of NUL-terminated strings.
tests/test_symtab_host.py parses the reference's own test/data/symboltable_test.bin
(tests/golden/symboltable_test.bin; its answers: test/symbol_table_test.cc:24-27) with the same
reader to pin the layout.

One name per output label of tests/golden/refmodel/wordloop.fst (make_fst_fixture.py: word ids
1..6; 0 is epsilon).
"""
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
WORDS = ["<eps>", "alder", "birch", "cedar", "douglas-fir", "elm", "fig"]


def encode(words):
    offsets, buf = [], b""
    for w in words:
        offsets.append(len(buf))
        buf += w.encode() + b"\0"
    body = struct.pack("<ii", len(words), len(buf)) + struct.pack("<%di" % len(words), *offsets) + buf
    return b"SYM0" + struct.pack("<i", len(body)) + body


def write(path):
    with open(path, "wb") as f:
        f.write(encode(WORDS))
    return len(WORDS)


if __name__ == "__main__":
    out = os.path.join(HERE, "refmodel", "wordloop_words.bin")
    print(out, "symbols:", write(out))
