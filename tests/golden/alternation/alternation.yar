rule alternation_hex {
 strings:
  $long_first = { AA BB CC DD ( 01 02 03 | 01 ) 02 03 }
  $short_first = { AB BB CC DD ( 01 | 01 02 03 ) 02 03 }
  $before = { ( 09 09 | 09 ) 02 03 A1 B2 C3 D4 }
  $three = { 11 22 33 44 ( 55 | 66 77 | 88 99 AA ) BB }
  $nested = { 21 22 23 24 ( 31 ( 41 | 42 43 ) | 32 ) 25 }
  $jump_in = { 51 52 53 54 ( 61 [1-2] 62 | 63 ) 55 }
  $wild = { 71 72 73 74 ( ?? 81 | ~82 83 | 8? 84 ) 75 }
  $meet = { 9A [0-4] B1 B2 B3 B4 [0-4] ( C1 | C2 ) }
  $run63 = { E1 E2 E3 E4 ( E5 | E6 ) [57] E7 }
  $run64 = { F1 E2 E3 E4 ( E5 | E6 ) [58] E7 }
  $run65 = { F2 E2 E3 E4 ( E5 | E6 ) [59] E7 }
  $insns65 = { D0 D1 D2 D3 ( 01 | 02 ) 03 04 05 06 07 08 09 0A 0B 0C 0D 0E 0F 10 11 12 13 14 15 16 17 18 19 1A 1B 1C 1D 1E 1F 20 21 22 23 24 25 26 27 28 29 2A 2B 2C 2D 2E 2F 30 31 32 33 34 35 36 37 38 39 3A }
  $far = { 7A 7B 7C 7D [0-100] 7E 7F }
 condition: any of them
}
rule alternation_text {
 strings:
  $animals = /(cat|dog|bird)house/
  $cls = /class[0-9]c/
  $ncls = /nocls[^0-9]z/
  $split_b = /klmn(x??)y/
  $split_a = /opqr(x?)y/
  $greedy = /ab.{1,3}cd/
  $ungreedy = /eb.{1,3}?cd/
  $greedy_s = /ib.{1,3}cd/s
  $plus = /zq+c/
  $boundary = /\bword(a|b)/
  $nocase = /(red|blue)fish/ nocase
  $wide = /(red|blue)bird/ wide
 condition: any of them
}
