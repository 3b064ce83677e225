// Stand-alone check of the host JPEG encoder (zh_jpeg_encode_host in zutis_amd/csrc/jpeg_host.hip over jpeg_codec.h — the arithmetic the
// device kernels compile) for the HOST sanitizers: every array of a call is a heap block of EXACTLY its bytes — `out` exactly out_bytes,
// which in the `overflow` case is three slots with a scan longer than its slot in the middle one — so that a read one past the pixels,
// a table or a descriptor, or a write one past a slot, the output or the lengths, is an AddressSanitizer report.  The inputs are the case
// files of tools/host/jpeg_enc_host_cases.py.  Checked: the call returns 0, the lengths are the definition's (the TRUE length where the
// scan does not fit, -1 for an image the call refuses), and every output byte is the definition's scan or still the fill.  CPU only, no
// GPU and no HIP runtime call; build and run: tools/README.md.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
  long long head[6];
  if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "ZHE1", 4) != 0 || std::fread(head, 8, 6, f) != 6) { std::printf("%s: no case file\n", path.c_str()); std::exit(2); }
  const long image_bytes = (long)head[0], B = (long)head[1], sub = (long)head[2], max_mcus = (long)head[3], out_bytes = (long)head[4], slot_bytes = (long)head[5];
  unsigned char* images = exact(f, (size_t)image_bytes);
  long long* img_off = (long long*)exact(f, (size_t)B * sizeof(long long));
  int* hw = (int*)exact(f, (size_t)B * 2 * sizeof(int));
  unsigned short* quant = (unsigned short*)exact(f, 128 * sizeof(unsigned short));
  long long* out_off = (long long*)exact(f, (size_t)B * sizeof(long long));
  int* want_len = (int*)exact(f, (size_t)B * sizeof(int));
  unsigned char* want = exact(f, (size_t)out_bytes);
  std::fclose(f);
  unsigned char* out = (unsigned char*)std::malloc((size_t)out_bytes);
  std::memset(out, 0xA5, (size_t)out_bytes);
  int* lengths = (int*)std::malloc((size_t)B * sizeof(int));
  const int rc = zh_jpeg_encode_host(images, image_bytes, img_off, hw, (int)B, (int)sub, max_mcus, quant, out_off, out, out_bytes, slot_bytes, lengths);
  ++g_calls;
  CHECK(rc == 0, "%s: returned %d", path.c_str(), rc);
  long over = 0, refused = 0, differ = 0;
  for (long b = 0; b < B; ++b) {
    CHECK(lengths[b] == want_len[b], "%s: image %ld has length %d, the definition %d", path.c_str(), b, lengths[b], want_len[b]);
    over += lengths[b] > slot_bytes;
    refused += lengths[b] < 0;
  }
  for (long i = 0; i < out_bytes; ++i) differ += out[i] != want[i];
  CHECK(differ == 0, "%s: %ld output bytes differ from the definition's", path.c_str(), differ);
  std::printf("%-18s B %ld, subsampling %ld, %ld image bytes, slot %ld, %ld longer than the slot, %ld refused\n", path.substr(path.find_last_of('/') + 1).c_str(), B, sub,
              image_bytes, slot_bytes, over, refused);
  std::free(images); std::free(img_off); std::free(hw); std::free(quant); std::free(out_off); std::free(want_len); std::free(want); std::free(out); std::free(lengths);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: jpeg_enc_host_check DIR (the directory tools/host/jpeg_enc_host_cases.py wrote)\n"); return 2; }
  const char* names[] = {"q1_444", "q1_420", "q50_444", "q50_420", "q90_444", "q90_420", "q100_444", "q100_420", "overflow", "refuse_grid", "refuse_out", "refuse_images"};
  for (const char* n : names) run_case(std::string(argv[1]) + "/" + n + ".zhe");
  std::printf("jpeg_enc_host_check: %d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
