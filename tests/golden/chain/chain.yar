// Hex strings that libyara splits into chains at a jump wider than 200 bytes:
// the chain replay of the match stage (tests/test_gpu_chain_matches.py);
// make_chain.py plants them.  Every part's atom is its run of four bytes.
rule chain_shapes
{
  strings:
    // two literal parts
    $two = { 10 11 12 13 [300-400] 14 15 16 17 }
    // three literal parts
    $three = { 20 21 22 23 [300-400] 24 25 26 27 [300-400] 28 29 2A 2B }
    // an unbounded jump
    $open = { 30 31 32 33 [300-] 34 35 36 37 }
    // a head with a wildcard before its atom: a hex part, one backward result
    $wild = { 4F ?? 40 41 42 43 [300-400] 45 46 47 48 }
    // a head with a jump before its atom: two backward results, a dirty chain
    $dirty = { 50 [1-3] 51 52 53 54 [300-400] 55 56 57 58 }
    // a head with one backward result at varying distances: two calls, one offset
    $vary = { 60 [1-30] 61 62 63 64 [300-400] 65 66 67 68 }
    // a regexp's chain (the compiler splits at an ungreedy /s dot range): never settled
    $regexp = /chn[0-9]{2}?.{300,400}?xyz/s
    // not a chain: a text string
    $text = "chain-literal"
  condition:
    any of them
}
