# dhtgpu_write_ids without its `net_valid = false` line: once an index query has rebuilt the set's K4 index,
# search_batch answers from the old crawl model's node order (same n: every read stays in bounds) where the header
# demands ENOIDS until dhtgpu_net_prepare.  tests/test_gpu_sequences.py's net-write_ids_* rows must fail on it.
# A test-sensitivity variant for tools/experiments/build_variant.sh: it changes no size, bound or pointer, and no
# test loads it (profiles/r14/sequences/notes.txt records the runs).
s = open("api.hip").read()
a = '    c->acc.index_valid = false;\n    c->net_valid = false;\n    c->invalidate_subs();\n'
assert s.count(a) == 1
s = s.replace(a, '    c->acc.index_valid = false;\n    c->invalidate_subs();\n')
open("api.hip", "w").write(s)
