// TEST INFRASTRUCTURE - blob_check <file>: the model blob's validator (minppo_amd/csrc/model_blob.hip) on its own, for a build under the
// host sanitizers (tests/test_blob_fuzz.py: g++ -fsanitize=address,undefined; nothing else of the library is linked).  The file holds
// blobs one after another, each behind its length in bytes (a 64-bit word); every blob is copied into a heap block of exactly its
// size, so that a read past its end is a read past the block's.  Prints one character per blob: 0 accepted, 1 refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "model_view.h"
#include "mppo_common.h"

namespace mppo {
char* last_error_buf() { static thread_local char buf[512]; return buf; }
}

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  if (!f) { fprintf(stderr, "usage: blob_check <file of length-prefixed blobs>\n"); return 2; }
  uint64_t n = 0;
  while (fread(&n, sizeof n, 1, f) == 1) {
    if (n > (1u << 30)) { fprintf(stderr, "blob_check: a blob of %llu bytes\n", (unsigned long long)n); return 2; }
    void* blob = malloc(n);
    if (!blob || (n > 0 && fread(blob, 1, n, f) != n)) { fprintf(stderr, "blob_check: no memory, or the file ends inside a blob\n"); return 2; }
    mppo::ModelView view;
    mppo::BlobDims dims{};
    int canon_words = 0;
    putchar(mppo::parse_model_blob(blob, n, &view, &dims, &canon_words) == MPPO_OK ? '0' : '1');
    free(blob);
  }
  fclose(f);
  putchar('\n');
  return 0;
}
