// Chains and alternation strings in one set of tables: the match stage with
// chains and alternations both on (tests/test_gpu_alternation.py).
rule both
{
  strings:
    // a settled chain of two literal parts
    $two = { 10 11 12 13 [300-400] 14 15 16 17 }
    // alternation strings: priority (stock: 9, not 7), two backward results
    $long_first = { AA BB CC DD ( 01 02 03 | 01 ) 02 03 }
    $before = { ( 09 09 | 09 ) 02 03 A1 B2 C3 D4 }
    // a settled chain whose head has a wildcard before its atom
    $wild = { 4F ?? 40 41 42 43 [300-400] 45 46 47 48 }
    // a chain with an alternation part: never settled
    $mixed = { 20 21 22 23 ( 31 | 32 33 ) [300-400] 24 25 26 27 }
    // backwards from its atom at offset 64 the long alternative is live at
    // position 64 (max_bytes_matched), the short one gives bytes_matched 63
    $edge = { ( A? | A2 A3 A3 ) [62] B1 B2 B3 B4 }
  condition:
    any of them
}
