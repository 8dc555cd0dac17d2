// Match lists past the keep mask: lists of 32, 33 and 70 entries, the last a shared-tail chain.
rule atom70 {
 strings:
  $s0 = "#q9%\x00A"
  $s1 = "#q9%\x00b" nocase
  $s2 = "#q9%\x00" fullword
  $s3 = { 23 71 39 25 00 [0-1] 4? }
  $s4 = /\#q9\%\x00{1,1}[A-D]/
  $s5 = "#q9%\x00\x00A"
  $s6 = "#q9%\x00\x00b" nocase
  $s7 = "#q9%\x00\x00C" fullword
  $s8 = { 23 71 39 25 00 [0-2] 42 }
  $s9 = /\#q9\%\x00{1,2}[B-E]/
  $s10 = "#q9%\x00\x00\x00A"
  $s11 = "#q9%\x00\x00\x00b" nocase
  $s12 = "#q9%\x00\x00\x00" fullword
  $s13 = { 23 71 39 25 00 [0-3] 4? }
  $s14 = /\#q9\%\x00{1,3}[C-F]/
  $s15 = "#q9%\x00\x00\x00\x00A"
  $s16 = "#q9%\x00\x00\x00\x00b" nocase
  $s17 = "#q9%\x00\x00\x00\x00C" fullword
  $s18 = { 23 71 39 25 00 [0-4] 44 }
  $s19 = /\#q9\%\x00{1,4}[A-D]/
  $s20 = "#q9%\x00\x00\x00\x00\x00A"
  $s21 = "#q9%\x00\x00\x00\x00\x00b" nocase
  $s22 = "#q9%\x00\x00\x00\x00\x00" fullword
  $s23 = { 23 71 39 25 00 [0-5] 4? }
  $s24 = /\#q9\%\x00{1,5}[B-E]/
  $s25 = "#q9%\x00\x00\x00\x00\x00\x00A"
  $s26 = "#q9%\x00\x00\x00\x00\x00\x00b" nocase
  $s27 = "#q9%\x00\x00\x00\x00\x00\x00C" fullword
  $s28 = { 23 71 39 25 00 [0-6] 46 }
  $s29 = /\#q9\%\x00{1,6}[C-F]/
  $s30 = "#q9%\x00\x00\x00\x00\x00\x00\x00A"
  $s31 = "#q9%\x00\x00\x00\x00\x00\x00\x00b" nocase
  $s32 = "#q9%\x00\x00\x00\x00\x00\x00\x00" fullword
  $s33 = { 23 71 39 25 00 [0-7] 4? }
  $s34 = /\#q9\%\x00{1,7}[A-D]/
  $s35 = "#q9%\x00\x00\x00\x00\x00\x00\x00\x00A"
  $s36 = "#q9%\x00\x00\x00\x00\x00\x00\x00\x00b" nocase
  $s37 = "#q9%\x00\x00\x00\x00\x00\x00\x00\x00C" fullword
  $s38 = { 23 71 39 25 00 [0-8] 42 }
  $s39 = /\#q9\%\x00{1,8}[B-E]/
  $s40 = "#q9%\x00B"
  $s41 = "#q9%\x00c" nocase
  $s42 = "#q9%\x00-" fullword
  $s43 = { 23 71 39 25 00 [0-9] 4? }
  $s44 = /\#q9\%\x00{1,1}[C-F]/
  $s45 = "#q9%\x00\x00B"
  $s46 = "#q9%\x00\x00c" nocase
  $s47 = "#q9%\x00\x00D" fullword
  $p0 = "\x00\x00#q9%\x00A"
  $p1 = "\x00\x00\x00\x00#q9%\x00"
 condition: any of them
}
rule tail3_0 {
 strings:
  $t0 = "q9%"
 condition: $t0
}
rule tail3_1 {
 strings:
  $t1 = "q9%" fullword
 condition: $t1
}
rule tail3_2 {
 strings:
  $t2 = "q9%" nocase
 condition: $t2
}
rule tail3_3 {
 strings:
  $t3 = "q9%"
 condition: $t3
}
rule tail3_4 {
 strings:
  $t4 = "q9%" fullword
 condition: $t4
}
rule tail3_5 {
 strings:
  $t5 = "q9%" nocase
 condition: $t5
}
rule tail3_6 {
 strings:
  $t6 = "q9%"
 condition: $t6
}
rule tail3_7 {
 strings:
  $t7 = "q9%" fullword
 condition: $t7
}
rule tail3_8 {
 strings:
  $t8 = "q9%" nocase
 condition: $t8
}
rule tail3_9 {
 strings:
  $t9 = "q9%"
 condition: $t9
}
rule tail3_10 {
 strings:
  $t10 = "q9%" fullword
 condition: $t10
}
rule tail3_11 {
 strings:
  $t11 = "q9%" nocase
 condition: $t11
}
rule tail3_12 {
 strings:
  $t12 = "q9%"
 condition: $t12
}
rule tail3_13 {
 strings:
  $t13 = "q9%"
 condition: $t13
}
rule tail3_14 {
 strings:
  $t14 = "q9%"
 condition: $t14
}
rule tail3_15 {
 strings:
  $t15 = "q9%"
 condition: $t15
}
rule tail2_0 { strings: $a = "9%" condition: $a }
rule tail2_1 { strings: $a = "9%" fullword condition: $a }
rule tail2_2 { strings: $a = "9%" condition: $a }
rule tail2_3 { strings: $a = "9%" fullword condition: $a }
rule atom32 {
 strings:
  $s0 = "Kx7!\x00A"
  $s1 = "Kx7!\x00b" nocase
  $s2 = "Kx7!\x00" fullword
  $s3 = { 4B 78 37 21 00 [0-1] 4? }
  $s4 = /Kx7\!\x00{1,1}[A-D]/
  $s5 = "Kx7!\x00\x00A"
  $s6 = "Kx7!\x00\x00b" nocase
  $s7 = "Kx7!\x00\x00C" fullword
  $s8 = { 4B 78 37 21 00 [0-2] 42 }
  $s9 = /Kx7\!\x00{1,2}[B-E]/
  $s10 = "Kx7!\x00\x00\x00A"
  $s11 = "Kx7!\x00\x00\x00b" nocase
  $s12 = "Kx7!\x00\x00\x00" fullword
  $s13 = { 4B 78 37 21 00 [0-3] 4? }
  $s14 = /Kx7\!\x00{1,3}[C-F]/
  $s15 = "Kx7!\x00\x00\x00\x00A"
  $s16 = "Kx7!\x00\x00\x00\x00b" nocase
  $s17 = "Kx7!\x00\x00\x00\x00C" fullword
  $s18 = { 4B 78 37 21 00 [0-4] 44 }
  $s19 = /Kx7\!\x00{1,4}[A-D]/
  $s20 = "Kx7!\x00\x00\x00\x00\x00A"
  $s21 = "Kx7!\x00\x00\x00\x00\x00b" nocase
  $s22 = "Kx7!\x00\x00\x00\x00\x00" fullword
  $s23 = { 4B 78 37 21 00 [0-5] 4? }
  $s24 = /Kx7\!\x00{1,5}[B-E]/
  $s25 = "Kx7!\x00\x00\x00\x00\x00\x00A"
  $s26 = "Kx7!\x00\x00\x00\x00\x00\x00b" nocase
  $s27 = "Kx7!\x00\x00\x00\x00\x00\x00C" fullword
  $s28 = { 4B 78 37 21 00 [0-6] 46 }
  $s29 = /Kx7\!\x00{1,6}[C-F]/
  $s30 = "Kx7!\x00\x00\x00\x00\x00\x00\x00A"
  $s31 = "Kx7!\x00\x00\x00\x00\x00\x00\x00b" nocase
 condition: any of them
}
rule atom33 {
 strings:
  $s0 = "Wm3&\x00A"
  $s1 = "Wm3&\x00b" nocase
  $s2 = "Wm3&\x00" fullword
  $s3 = { 57 6D 33 26 00 [0-1] 4? }
  $s4 = /Wm3\&\x00{1,1}[A-D]/
  $s5 = "Wm3&\x00\x00A"
  $s6 = "Wm3&\x00\x00b" nocase
  $s7 = "Wm3&\x00\x00C" fullword
  $s8 = { 57 6D 33 26 00 [0-2] 42 }
  $s9 = /Wm3\&\x00{1,2}[B-E]/
  $s10 = "Wm3&\x00\x00\x00A"
  $s11 = "Wm3&\x00\x00\x00b" nocase
  $s12 = "Wm3&\x00\x00\x00" fullword
  $s13 = { 57 6D 33 26 00 [0-3] 4? }
  $s14 = /Wm3\&\x00{1,3}[C-F]/
  $s15 = "Wm3&\x00\x00\x00\x00A"
  $s16 = "Wm3&\x00\x00\x00\x00b" nocase
  $s17 = "Wm3&\x00\x00\x00\x00C" fullword
  $s18 = { 57 6D 33 26 00 [0-4] 44 }
  $s19 = /Wm3\&\x00{1,4}[A-D]/
  $s20 = "Wm3&\x00\x00\x00\x00\x00A"
  $s21 = "Wm3&\x00\x00\x00\x00\x00b" nocase
  $s22 = "Wm3&\x00\x00\x00\x00\x00" fullword
  $s23 = { 57 6D 33 26 00 [0-5] 4? }
  $s24 = /Wm3\&\x00{1,5}[B-E]/
  $s25 = "Wm3&\x00\x00\x00\x00\x00\x00A"
  $s26 = "Wm3&\x00\x00\x00\x00\x00\x00b" nocase
  $s27 = "Wm3&\x00\x00\x00\x00\x00\x00C" fullword
  $s28 = { 57 6D 33 26 00 [0-6] 46 }
  $s29 = /Wm3\&\x00{1,6}[C-F]/
  $s30 = "Wm3&\x00\x00\x00\x00\x00\x00\x00A"
  $s31 = "Wm3&\x00\x00\x00\x00\x00\x00\x00b" nocase
  $s32 = "Wm3&\x00\x00\x00\x00\x00\x00\x00" fullword
 condition: any of them
}
rule k5_0 { strings: $a = "~" condition: $a }
rule k5_1 { strings: $a = "~" condition: $a }
rule k5_2 { strings: $a = "~" condition: $a }
rule k5_3 { strings: $a = "~" condition: $a }
rule k5_4 { strings: $a = "~" condition: $a }
rule k30_0 { strings: $a = "^" condition: $a }
rule k30_1 { strings: $a = "^" condition: $a }
rule k30_2 { strings: $a = "^" condition: $a }
rule k30_3 { strings: $a = "^" condition: $a }
rule k30_4 { strings: $a = "^" condition: $a }
rule k30_5 { strings: $a = "^" condition: $a }
rule k30_6 { strings: $a = "^" condition: $a }
rule k30_7 { strings: $a = "^" condition: $a }
rule k30_8 { strings: $a = "^" condition: $a }
rule k30_9 { strings: $a = "^" condition: $a }
rule k30_10 { strings: $a = "^" condition: $a }
rule k30_11 { strings: $a = "^" condition: $a }
rule k30_12 { strings: $a = "^" condition: $a }
rule k30_13 { strings: $a = "^" condition: $a }
rule k30_14 { strings: $a = "^" condition: $a }
rule k30_15 { strings: $a = "^" condition: $a }
rule k30_16 { strings: $a = "^" condition: $a }
rule k30_17 { strings: $a = "^" condition: $a }
rule k30_18 { strings: $a = "^" condition: $a }
rule k30_19 { strings: $a = "^" condition: $a }
rule k30_20 { strings: $a = "^" condition: $a }
rule k30_21 { strings: $a = "^" condition: $a }
rule k30_22 { strings: $a = "^" condition: $a }
rule k30_23 { strings: $a = "^" condition: $a }
rule k30_24 { strings: $a = "^" condition: $a }
rule k30_25 { strings: $a = "^" condition: $a }
rule k30_26 { strings: $a = "^" condition: $a }
rule k30_27 { strings: $a = "^" condition: $a }
rule k30_28 { strings: $a = "^" condition: $a }
rule k30_29 { strings: $a = "^" condition: $a }
rule k33_0 { strings: $a = "|" fullword condition: $a }
rule k33_1 { strings: $a = "|" condition: $a }
rule k33_2 { strings: $a = "|" fullword condition: $a }
rule k33_3 { strings: $a = "|" condition: $a }
rule k33_4 { strings: $a = "|" fullword condition: $a }
rule k33_5 { strings: $a = "|" condition: $a }
rule k33_6 { strings: $a = "|" fullword condition: $a }
rule k33_7 { strings: $a = "|" condition: $a }
rule k33_8 { strings: $a = "|" fullword condition: $a }
rule k33_9 { strings: $a = "|" condition: $a }
rule k33_10 { strings: $a = "|" fullword condition: $a }
rule k33_11 { strings: $a = "|" condition: $a }
rule k33_12 { strings: $a = "|" fullword condition: $a }
rule k33_13 { strings: $a = "|" condition: $a }
rule k33_14 { strings: $a = "|" fullword condition: $a }
rule k33_15 { strings: $a = "|" condition: $a }
rule k33_16 { strings: $a = "|" fullword condition: $a }
rule k33_17 { strings: $a = "|" condition: $a }
rule k33_18 { strings: $a = "|" fullword condition: $a }
rule k33_19 { strings: $a = "|" condition: $a }
rule k33_20 { strings: $a = "|" fullword condition: $a }
rule k33_21 { strings: $a = "|" condition: $a }
rule k33_22 { strings: $a = "|" fullword condition: $a }
rule k33_23 { strings: $a = "|" condition: $a }
rule k33_24 { strings: $a = "|" fullword condition: $a }
rule k33_25 { strings: $a = "|" condition: $a }
rule k33_26 { strings: $a = "|" fullword condition: $a }
rule k33_27 { strings: $a = "|" condition: $a }
rule k33_28 { strings: $a = "|" fullword condition: $a }
rule k33_29 { strings: $a = "|" condition: $a }
rule k33_30 { strings: $a = "|" fullword condition: $a }
rule k33_31 { strings: $a = "|" condition: $a }
rule k33_32 { strings: $a = "|" fullword condition: $a }
