// Hex strings whose jumps carry the position set past 64 positions: the
// wave-wide path of the match stage's hex class (tests/test_gpu_hex_wide.py);
// make_hexwide.py plants them.  Every string's atom is its run of four bytes.
rule hexwide_shapes
{
  strings:
    // one forward jump past a word of the set
    $fwd = { A1 A2 A3 A4 [0-100] A5 A6 }
    // the same tail and one byte more: a continuation that would end past the buffer
    $fwd_end = { A7 A8 A9 AA [0-100] A5 A6 A5 }
    // backward jumps: several starts over two words; shifts by 64, by 70, to 199
    $back = { B5 [0-100] B1 B2 B3 B4 }
    $back64 = { C5 [64-128] C1 C2 C3 C4 }
    $back70 = { D5 [70-199] D1 D2 D3 D4 }
    // two backward jumps: three words live
    $two = { E5 [0-100] E6 [0-100] E1 E2 E3 E4 }
    // two forward jumps, the second run from several positions: the order of
    // the reference's list decides -- wide, and the narrow shape
    $order = { F1 F2 F3 F4 [0-80] F5 [2-70] F6 }
    $order_narrow = { 71 72 73 74 [0-3] 75 [2-5] 76 }
    // 21 jumps of 200: the set reaches YR_RE_SCAN_LIMIT, the program is past 48 bytes
    $limit = { 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200]
               90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200]
               90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200] 90 [0-200]
               9A 9B 9C 9D }
    // not in the class: a chained string, a text string, a regexp
    $chain = { AA BB CC DD [300-400] EE FF 11 22 }
    $text = "hexwide-literal"
    $regexp = /hw[0-9]{2}xyz/
  condition:
    any of them
}
