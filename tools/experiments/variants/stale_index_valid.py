# dhtgpu_write_ids without its `index_valid = false` line: the set's K4 index keeps answering from the ids it was
# built over (same n: every read stays in bounds).  tests/test_gpu_sequences.py's index-write_ids_* rows must fail on it.
# A test-sensitivity variant for tools/experiments/build_variant.sh: it changes no size, bound or pointer, and no
# test loads it (profiles/r14/sequences/notes.txt records the runs).
s = open("api.hip").read()
a = '    c->index_valid = false;\n    c->acc.index_valid = false;\n    c->net_valid = false;\n    c->invalidate_subs();\n'
assert s.count(a) == 1
s = s.replace(a, '    c->acc.index_valid = false;\n    c->net_valid = false;\n    c->invalidate_subs();\n')
open("api.hip", "w").write(s)
