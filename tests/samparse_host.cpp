// samparse_host.cpp — elprep_amd/csrc/samparse.hpp behind C functions, for tests/test_samparse_cpu.py.  The header is host-and-device
// code: this file is built by the host compiler alone.
//   With -DSAMPARSE_MAIN it is a program of its own (for a build with -fsanitize=address,undefined): it reads a token file - one token
// per line as "<kind>\t<token>", kind = i8 i16 i32 i64 u8 u16 u32 (integers), f (float32), c (CIGAR) - and prints one line per token:
// "<reason> <value>" (integers: 0 / 1 for ok / error and the value; floats: the reason and the bits in hex; CIGAR: the reason and the
// operations as hex words).  `python -m tests.test_samparse_cpu write FILE` writes the tokens of the tests, `... check FILE OUT` compares.
#include "../elprep_amd/csrc/samparse.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace elp::samparse;

extern "C" {

int samparse_int(const uint8_t *s, uint32_t n, uint32_t bits, int is_signed, int64_t *out) { return parse_int(s, n, bits, is_signed != 0, out) ? 1 : 0; }
uint32_t samparse_f32(const uint8_t *s, uint32_t n, uint32_t *bits) { return parse_f32(s, n, bits); }
uint32_t samparse_cigar(const uint8_t *s, uint32_t n, uint32_t *ops, uint32_t *n_ops) { return parse_cigar(s, n, ops, n_ops); }
uint32_t samparse_nibble(uint8_t c) { return base_nibble(c); }
uint32_t samparse_entry(uint8_t st, const uint8_t *s, uint32_t n, uint32_t *value) { return parse_entry(st, s, n, value); }
uint32_t samparse_int_store(int64_t v, uint8_t *type) { return int_store(v, type); }
uint32_t samparse_unsupported_from(void) { return R_UNSUPPORTED; }

// n float tokens at once: token k = text[off[k] .. off[k + 1]); its bits and reason
void samparse_f32_many(const uint8_t *text, const uint32_t *off, uint64_t n, uint32_t *bits, uint8_t *reason) {
  for (uint64_t k = 0; k < n; k++) {
    bits[k] = 0;
    reason[k] = (uint8_t)parse_f32(text + off[k], off[k + 1] - off[k], &bits[k]);
  }
}

}  // extern "C"

#ifdef SAMPARSE_MAIN
int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s TOKENS\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::string line;
  std::vector<uint32_t> ops(65536);
  int ch;
  unsigned long long n_lines = 0;
  for (;;) {
    line.clear();
    while ((ch = fgetc(f)) != EOF && ch != '\n') line.push_back((char)ch);
    if (ch == EOF && line.empty()) break;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos) { fprintf(stderr, "line %llu: no tab\n", n_lines); return 2; }
    const std::string kind = line.substr(0, tab);
    // (a copy of exactly the token's bytes: a read past its end is a heap overflow the sanitizer sees)
    std::vector<uint8_t> tok(line.begin() + (long)tab + 1, line.end());
    const uint8_t *s = tok.data();
    const uint32_t n = (uint32_t)tok.size();
    if (kind == "f") {
      uint32_t bits = 0;
      const uint32_t r = parse_f32(s, n, &bits);
      printf("%u %08x\n", r, r ? 0u : bits);
    } else if (kind == "c") {
      uint32_t cnt = 0;
      const uint32_t r = parse_cigar(s, n, ops.data(), &cnt);
      printf("%u", r);
      for (uint32_t k = 0; !r && k < cnt; k++) printf(" %x", ops[k]);
      printf("\n");
    } else {
      const bool is_signed = kind[0] == 'i';
      int64_t v = 0;
      const bool ok = parse_int(s, n, (uint32_t)atoi(kind.c_str() + 1), is_signed, &v);
      printf("%d %lld\n", ok ? 0 : 1, ok ? (long long)v : 0ll);
    }
    n_lines++;
    if (ch == EOF) break;
  }
  fclose(f);
  fprintf(stderr, "%llu tokens\n", n_lines);
  return 0;
}
#endif
