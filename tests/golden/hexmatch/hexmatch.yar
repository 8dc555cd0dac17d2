// Hex strings whose calls the match stage's hex class measures
// (tests/test_gpu_hex_matches.py); make_hexmatch.py plants them.
rule hexmatch_shapes
{
  strings:
    // the atom lies behind two jumps: the backward run yields several offsets
    $two_back = { C1 [0-3] C2 [0-3] C3 C4 C5 C6 C7 }
    // several continuations after the atom: the forward run keeps the shortest
    $shortest = { D1 D2 D3 D4 [0-4] D5 D6 }
    // two atoms can reach back to one start
    $same_start = { E1 [0-4] E2 E3 E4 E5 }
    // wider than the device's window of 64 positions, below the chaining threshold
    $wide = { F1 F2 F3 F4 [0-100] F5 F6 }
    $masked = { 9? A? B1 ?? B2 B3 B4 [1-2] B5 }
    $both_sides = { 81 82 83 84 [2-6] 85 [0-2] 86 87 88 89 }
    // not in the class: a chained string, a text string, a regexp
    $chain = { AA BB CC DD [300-400] EE FF 11 22 }
    $text = "hexmatch-literal"
    $regexp = /hm[0-9]{2}xyz/
  condition:
    any of them
}
