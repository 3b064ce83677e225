// Stand-alone check of the host COCO RLE entry points (zutis_amd/csrc/rle_host.hip over rle_codec.h) for the HOST sanitizers: every call
// gets heap buffers of EXACTLY the bytes it may touch — the string's length, and one byte less, which must give -1 — so that a read or
// write one past an end is an AddressSanitizer report.  CPU only, no GPU and no HIP runtime call; build and run: tools/README.md.
// The strings are checked against the literals worked out in tests/test_rle.py's docstring and by reading them back (a decoder is
// not a copy of the emitter); tests/test_rle.py holds the same entry points against the Python restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/zutis_hip.h"

static int g_fail = 0, g_calls = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

typedef std::vector<long long> Counts;

// heap copy of exactly v.size() elements (a null pointer for none would hide nothing: malloc(0) is a valid zero-byte block for ASan)
template <class T> static T* exact(const std::vector<T>& v) {
  T* p = (T*)std::malloc(v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// the reader: characters -> run lengths (pycocotools rleFrString)
static Counts read_back(const std::string& s) {
  Counts c;
  size_t p = 0;
  while (p < s.size()) {
    long long x = 0;
    int k = 0;
    bool more = true;
    while (more) {
      const long long ch = s[p] - 48;
      x |= (ch & 0x1f) << (5 * k);
      more = (ch & 0x20) != 0;
      ++p; ++k;
      if (!more && (ch & 0x10)) x |= (long long)(~0ULL << (5 * k));
    }
    if (c.size() > 2) x += c[c.size() - 2];
    c.push_back(x);
  }
  return c;
}

// runs `call(out, cap)` with a roomy buffer to learn the length, then with exactly that many bytes and with one less
template <class F> static std::string at_capacities(const char* what, F call) {
  std::vector<char> big(1 << 16);
  const long n = call(big.data(), (long)big.size());
  ++g_calls;
  CHECK(n >= 0, "%s: %ld with room to spare", what, n);
  if (n < 0) return "";
  char* tight = (char*)std::malloc((size_t)n);
  const long m = call(tight, n);
  CHECK(m == n && std::memcmp(tight, big.data(), (size_t)n) == 0, "%s: %ld at exact capacity %ld", what, m, n);
  std::free(tight);
  if (n > 0) {
    char* shorter = (char*)std::malloc((size_t)n - 1);
    const long r = call(shorter, n - 1);
    CHECK(r == -1, "%s: %ld at capacity %ld, -1 expected", what, r, n - 1);
    std::free(shorter);
  }
  g_calls += 2;
  return std::string(big.data(), (size_t)n);
}

static std::string counts_string(const Counts& c) {
  long long* h = exact(c);
  const std::string s = at_capacities("counts_to_string", [&](char* o, long cap) { return zh_rle_counts_to_string_host(h, (long)c.size(), o, cap); });
  std::free(h);
  CHECK(read_back(s) == c, "counts_to_string: \"%s\" does not read back", s.c_str());
  return s;
}

// mask [h, w] row-major from column-major runs (the run of zeros first)
static std::vector<unsigned char> mask_from_runs(int h, int w, const Counts& runs) {
  std::vector<unsigned char> m((size_t)h * w);
  long pos = 0;
  unsigned char val = 0;
  for (long long r : runs) {
    for (long long i = 0; i < r; ++i, ++pos) m[(size_t)(pos % h) * w + pos / h] = val ? 255 : 0;       // any non-zero byte is set
    val ^= 1;
  }
  CHECK(pos == (long)h * w, "runs sum to %ld, mask has %ld pixels", pos, (long)h * w);
  return m;
}

static std::string mask_string(int h, int w, const std::vector<unsigned char>& m) {
  unsigned char* d = exact(m);
  const std::string s = at_capacities("encode", [&](char* o, long cap) { return zh_rle_encode_host(d, h, w, o, cap); });
  std::free(d);
  return s;
}

// the transition list of column-major runs: positions where the value changes, and the value of pixel 0
static void transitions(const Counts& runs, std::vector<int>& pos, int& first) {
  first = !runs.empty() && runs[0] == 0;
  long long at = 0;
  for (size_t k = 0; k + 1 < runs.size(); ++k) { at += runs[k]; if (at > 0) pos.push_back((int)at); }
}

struct Vec { int h, w; Counts runs; const char* chars; };

int main() {
  // ---- the vectors worked out in tests/test_rle.py (tests/golden/rle_vectors.json) and its docstring's values
  const Vec vecs[] = {
    {3, 3, {9}, "9"}, {2, 2, {0, 4}, "04"}, {4, 4, {5, 1, 10}, "51:"}, {8, 12, {3, 2, 40, 1, 50}, "32X1O:"},
    {64, 47, {0, 1000, 5, 3, 2000}, "0Xo05kPO[n1"}, {4, 16, {31, 1, 32}, "o01P1"}, {5, 8, {16, 8, 16}, "`08`0"},
  };
  const struct { long long v; const char* chars; } worked[] = {{9, "9"}, {40, "X1"}, {-1, "O"}, {1000, "Xo0"}, {-997, "kPO"}, {1995, "[n1"},
                                                               {31, "o0"}, {16, "`0"}, {0, "0"}};
  for (const Vec& v : vecs) {
    CHECK(mask_string(v.h, v.w, mask_from_runs(v.h, v.w, v.runs)) == v.chars, "encode: %dx%d is not \"%s\"", v.h, v.w, v.chars);
    CHECK(counts_string(v.runs) == v.chars, "counts_to_string: not \"%s\"", v.chars);
  }
  for (const auto& w : worked) {
    const std::string s = w.v >= 0 ? counts_string({w.v}) : counts_string({5, -w.v, 7, 0});
    CHECK(s.size() >= std::strlen(w.chars) && s.substr(s.size() - std::strlen(w.chars)) == w.chars, "value %lld is not \"%s\"", w.v, w.chars);
  }
  // ---- values on both sides of every character-count boundary, plain, as the positive and as the negative delta against counts[k - 2]
  const long long edges[] = {0, 15, 16, 31, 32, (1LL << 24) - 1, 1LL << 24, (1LL << 31) - 1};
  const int nchar[] = {1, 1, 2, 2, 2, 5, 6, 7};
  for (size_t i = 0; i < sizeof(edges) / sizeof(edges[0]); ++i) {
    const long long v = edges[i];
    CHECK((int)counts_string({v}).size() == nchar[i], "%lld takes %zu characters", v, counts_string({v}).size());
    counts_string({5, 0, 7, v});
    counts_string({5, v, 7, 0});
    counts_string({v, v, v, v, v});
    // the same values from a transition list: one transition at pixel 1 (run 1 = v), and runs 1, v + 1, 1, 1 (the last stored as -v)
    if (v >= 1 && v + 4 < (1LL << 31)) {
      for (const Counts& runs : {Counts{1, v}, Counts{1, v + 1, 1, 1}}) {
        std::vector<int> pos; int first;
        transitions(runs, pos, first);
        long long hw = 0;
        for (long long r : runs) hw += r;
        const std::vector<int> nr = {(int)pos.size(), first};
        int *hp = exact(pos), *hn = exact(nr);
        long long* off = (long long*)std::malloc(2 * sizeof(long long));
        const std::string s = at_capacities("from_transitions", [&](char* o, long cap) {
          return zh_rle_from_transitions_host(hp, (long)pos.size(), 0, hn, 1, (long)hw, o, cap, off); });
        CHECK(read_back(s) == runs && off[0] == 0 && off[1] == (long long)s.size(), "from_transitions: value %lld", v);
        std::free(hp); std::free(hn); std::free(off);
      }
    }
  }
  // ---- n = 0: an empty mask is the one run of length 0, no counts and no masks are the empty string
  CHECK(mask_string(0, 5, {}) == "0" && mask_string(3, 0, {}) == "0", "encode: an empty mask is not \"0\"");
  CHECK(counts_string({}) == "", "counts_to_string: n = 0");
  {
    long long* off = (long long*)std::malloc(sizeof(long long));
    std::vector<int> none;
    int *hp = exact(none), *hn = exact(none);
    CHECK(at_capacities("from_transitions n = 0", [&](char* o, long cap) { return zh_rle_from_transitions_host(hp, 4, 1, hn, 0, 1024, o, cap, off); }) == "" &&
          off[0] == 0, "from_transitions: n = 0");
    std::free(hp); std::free(hn); std::free(off);
  }
  // ---- the strided and the packed form of the transition list, with one row over `stride` (an empty string; the packed list holds
  //      `stride` entries of it, which the next row must skip)
  {
    const std::vector<Counts> rows = {{3, 2, 40, 1, 50}, {0, 7, 1, 1, 1, 1, 1, 84}, {96}, {0, 96}, {31, 1, 32, 16, 16}};
    const long stride = 4, hw = 96;
    std::vector<int> strided(rows.size() * stride, 0), packed, nr;
    std::string want;
    std::vector<long long> want_off;
    for (size_t i = 0; i < rows.size(); ++i) {
      std::vector<int> pos; int first;
      transitions(rows[i], pos, first);
      nr.push_back((int)pos.size()); nr.push_back(first);
      for (size_t k = 0; k < pos.size() && k < (size_t)stride; ++k) { strided[i * stride + k] = pos[k]; packed.push_back(pos[k]); }
      want_off.push_back((long long)want.size());
      if ((long)pos.size() <= stride) want += counts_string(rows[i]);
    }
    want_off.push_back((long long)want.size());
    CHECK(nr[2] == 6, "the second row is meant to have more transitions than the stride");
    for (int is_packed = 0; is_packed < 2; ++is_packed) {
      int *hp = exact(is_packed ? packed : strided), *hn = exact(nr);
      long long* off = (long long*)std::malloc((rows.size() + 1) * sizeof(long long));
      const std::string s = at_capacities(is_packed ? "from_transitions packed" : "from_transitions strided", [&](char* o, long cap) {
        return zh_rle_from_transitions_host(hp, stride, is_packed, hn, (long)rows.size(), hw, o, cap, off); });
      CHECK(s == want && std::vector<long long>(off, off + rows.size() + 1) == want_off, "from_transitions: %s form", is_packed ? "packed" : "strided");
      std::free(hp); std::free(hn); std::free(off);
    }
  }
  std::printf("rle_host_check: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
