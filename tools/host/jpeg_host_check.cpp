// Stand-alone check of the host JPEG decoders (zutis_amd/csrc/jpeg_host.hip over jpeg_codec.h — the codec the device kernels compile:
// zh_jpeg_decode_host, one segment after the other, and zh_jpeg_decode_split_host, every segment split into chunks) for
// the HOST sanitizers: every array of a call is a heap block of EXACTLY its bytes, so that a read one past a segment, a table or a
// descriptor row, or a write one past the output or the status array, is an AddressSanitizer report.  The inputs are the case files of
// tools/host/jpeg_host_cases.py: two good files, each damaged scan of the tests between two good files (at 16-byte chunks and at the
// shipped chunk size), a two-sequence file with one synchronising pass, and chunk rows that lie.  Every case runs through BOTH entries.
// Checked: the call returns 0, an image expected to fail under that entry has a non-zero status, every other one status 0 and the
// definition's pixels, and not one output byte outside the good images' pixels and the failed images' own ranges differs from the
// fill.  CPU only, no GPU and no HIP runtime call; build and run: tools/README.md.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/zutis_hip.h"

// the library's error text lives in capi.hip, which is not linked here
void zh_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  std::fputc('\n', stderr);
}

static int g_fail = 0, g_calls = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a heap block of exactly n bytes read from f
static unsigned char* exact(std::FILE* f, size_t n) {
  unsigned char* p = (unsigned char*)std::malloc(n);
  if (n && std::fread(p, 1, n, f) != n) { std::printf("short case file\n"); std::exit(2); }
  return p;
}

static void run_case(const std::string& path) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { std::printf("cannot open %s\n", path.c_str()); std::exit(2); }
  char magic[4];
  long long head[9];
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "ZHJ2", 4) != 0 || std::fread(head, 8, 9, f) != 9) { std::printf("%s: no case file\n", path.c_str()); std::exit(2); }
  const long scan_bytes = (long)head[0], n_segments = (long)head[1], B = (long)head[2], n_sets = (long)head[3], n_blocks = (long)head[4], out_bytes = (long)head[5];
  const long n_chunks = (long)head[6], chunk_bytes = (long)head[7], passes = (long)head[8];
  unsigned char* scan = exact(f, (size_t)scan_bytes);
  int* segments = (int*)exact(f, (size_t)n_segments * ZH_JPEG_SEGMENT_WORDS * sizeof(int));
  int* images = (int*)exact(f, (size_t)B * ZH_JPEG_IMAGE_WORDS * sizeof(int));
  unsigned char* tables = exact(f, (size_t)n_sets * ZH_JPEG_TABLE_SET_BYTES);
  int* chunks = (int*)exact(f, (size_t)n_chunks * ZH_JPEG_CHUNK_WORDS * sizeof(int));
  int* damaged = (int*)exact(f, (size_t)B * sizeof(int));
  unsigned char* want = exact(f, (size_t)out_bytes);
  std::fclose(f);
  const std::string name = path.substr(path.find_last_of('/') + 1);
  for (int split = 0; split < 2; ++split) {
    unsigned char* out = (unsigned char*)std::malloc((size_t)out_bytes);
    std::memset(out, 0xA5, (size_t)out_bytes);
    int* status = (int*)std::malloc((size_t)B * sizeof(int));
    const int rc = split ? zh_jpeg_decode_split_host(scan, scan_bytes, segments, (int)n_segments, chunks, n_chunks, (int)chunk_bytes, (int)passes, images, (int)B,
                                                     tables, (int)n_sets, n_blocks, out, out_bytes, status)
                         : zh_jpeg_decode_host(scan, scan_bytes, segments, (int)n_segments, images, (int)B, tables, (int)n_sets, n_blocks, out, out_bytes, status);
    ++g_calls;
    CHECK(rc == 0, "%s: returned %d", path.c_str(), rc);
    std::vector<char> skip((size_t)out_bytes, 0);                // a failed image's own pixels: whatever the decoder left there
    for (long b = 0; b < B; ++b) {
      const int* r = images + b * ZH_JPEG_IMAGE_WORDS;
      const bool fails = (damaged[b] >> split) & 1;
      CHECK(fails ? status[b] != 0 : status[b] == 0, "%s (%s): image %ld has status %d", path.c_str(), split ? "split" : "serial", b, status[b]);
      if (damaged[b])
        for (long i = 16L * r[9], e = i + 3L * r[0] * r[1]; i < e && i < out_bytes; ++i) skip[(size_t)i] = 1;
    }
    long differ = 0;
    for (long i = 0; i < out_bytes; ++i) differ += !skip[(size_t)i] && out[i] != want[i];
    CHECK(differ == 0, "%s (%s): %ld output bytes differ from the definition's", path.c_str(), split ? "split" : "serial", differ);
    std::printf("%-18s %-6s B %ld, %ld segments, %ld scan bytes, %ld chunks of %ld, %ld passes, status", name.c_str(), split ? "split" : "serial", B, n_segments,
                scan_bytes, n_chunks, chunk_bytes, passes);
    for (long b = 0; b < B; ++b) std::printf(" %d", status[b]);
    std::printf("\n");
    std::free(out); std::free(status);
  }
  std::free(scan); std::free(segments); std::free(images); std::free(tables); std::free(chunks); std::free(damaged); std::free(want);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: jpeg_host_check DIR (the directory tools/host/jpeg_host_cases.py wrote)\n"); return 2; }
  const char* names[] = {"good", "cut", "ff00", "marker", "zeros", "dri", "good_d", "cut_d", "ff00_d", "marker_d", "zeros_d", "dri_d",
                         "one_pass", "lie_offset", "lie_segment", "lie_unstuffed", "lie_first"};
  for (const char* n : names) run_case(std::string(argv[1]) + "/" + n + ".zhj");
  std::printf("jpeg_host_check: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
