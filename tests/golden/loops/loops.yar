rule loops_in {
 strings:
  $plus = /pLg1b+/
  $star = /sTg2b*/
  $plus_u = /pLu3b+?/
  $star_u = /sTu4b*?/
  $alt = /Lp5(ab|c)+d/
  $php = /[a-z]+\.php/
  $run = /Rn6!a+z/
  $dot = /D0t!.*;/
  $line = /N1a.*b!/
  $line_s = /N2a.*b!/s
  $coll_g = /x.*\.php/
  $coll_u = /y.*?\.php/
 condition: any of them
}
rule loops_out {
 strings:
  $eps = /(a*)*b/
  $count = /q[0-9]{2,8}z/
  $bound = /\bw+x/
  $any = /ab.{1,3}c+d/
  $nocase = /nC7a+b/ nocase
  $wide = /wD8a+b/ wide
  $big = /A0B1C2D3E4F5G6H7I8J9K0L1M2N3O4P5Q6R7S8T9U0V1W2X3Y4Z5A6B7C8D9E0F1G2H3I4J5K6L7M8N9O0P1Q2R3S4T5U6V7W8X9Y0Z1A2B3C4D5E6F7G8H9I0J1K2L3M4N5O6P7Q8R9+/
  $animals = /(cat|dog)house/
 condition: any of them
}
