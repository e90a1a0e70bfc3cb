// Driver of the host emulation of csrc/resample.hip: `oneshot` runs mi355asr_resample on files of raw arrays, `stream` feeds one slot
// of mi355asr_resample_streams_* packet by packet and flushes it, from position 0 or from the position given after the output file
// (a fresh slot placed there: what lies before it is zero).  RESAMPLE_SOURCE is the kernel file with its include of model.h
// replaced by shim.h and its LDS declaration by the emulation's block (the test makes that copy).
#include RESAMPLE_SOURCE
#include <string>
static std::vector<char> rd(const char* p) { FILE* f = fopen(p, "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); std::vector<char> b(n); if (n) fread(b.data(), 1, n, f); fclose(f); return b; }
static void wr(const char* p, const void* d, size_t n) { FILE* f = fopen(p, "wb"); fwrite(d, 1, n, f); fclose(f); }
int main(int argc, char** argv) {
  std::string mode = argv[1];
  int up = atoi(argv[2]), down = atoi(argv[3]);
  auto tab = rd(argv[4]);
  float* filt = (float*)aligned_alloc(16, tab.size()); memcpy(filt, tab.data(), tab.size());
  if (mode == "oneshot") {
    auto xb = rd(argv[5]); int dtype = argv[6][0] == 'i' ? MI355ASR_DT_I16 : MI355ASR_DT_F32;
    int B = atoi(argv[7]); long Lpad = atol(argv[8]), Opad = atol(argv[9]); auto lb = rd(argv[10]);
    bool misalign = argc > 12 && argv[12][0] == 'm';
    char* xraw = (char*)aligned_alloc(16, ((xb.size() + 31) & ~15ul) + 16);
    char* x = xraw + (misalign ? 4 : 0); memcpy(x, xb.data(), xb.size());
    // exact-size buffer so that a read past the batch shows up
    char* xe = (char*)malloc(xb.size()); memcpy(xe, xb.data(), xb.size());
    const void* xin = misalign ? (const void*)x : (((uintptr_t)xe & 15) == 0 ? (const void*)xe : (const void*)x);
    float* y = (float*)aligned_alloc(16, ((size_t)B * Opad * 4 + 15) & ~15ul);
    for (size_t i = 0; i < (size_t)B * Opad; ++i) y[i] = 12345.0f;
    int rc = mi355asr_resample(xin, dtype, (const int32_t*)lb.data(), B, Lpad, up, down, filt, y, Opad, nullptr);
    if (rc) { fprintf(stderr, "rc %d %s\n", rc, g_err); return 2; }
    wr(argv[11], y, (size_t)B * Opad * 4);
    free(xraw); free(xe); free(y);
  } else {
    auto xb = rd(argv[5]); const float* x = (const float*)xb.data(); long total = xb.size() / 4;
    int max_packet = atoi(argv[6]); auto sb = rd(argv[7]); const int32_t* sizes = (const int32_t*)sb.data(); int ns = sb.size() / 4;
    const int nstreams = 3, slot = 1;
    size_t stb, wsb; int32_t oc;
    if (mi355asr_resample_streams_bytes(up, down, nstreams, max_packet, &stb, &wsb, &oc)) { fprintf(stderr, "%s\n", g_err); return 2; }
    char* st = (char*)malloc(stb); memset(st, 0xff, stb); char* ws = (char*)malloc(wsb);
    if (mi355asr_resample_streams_reset(st, up, down, nstreams, max_packet, &slot, 1, nullptr)) return 2;
    const int64_t start = argc > 9 ? atoll(argv[9]) : 0;
    std::vector<float> out; int64_t pos = start; float* y = (float*)malloc((size_t)oc * 4);
    for (int i = 0; i <= ns; ++i) {
      int flush = i == ns; int32_t P = flush ? 0 : sizes[i], n_out = 0;
      float* pk = (float*)malloc(std::max(P, 1) * 4); if (P) memcpy(pk, x + (pos - start), P * 4);
      int rc = mi355asr_resample_streams_step(st, up, down, nstreams, max_packet, filt, &slot, &pos, &P, 1, flush, flush ? nullptr : pk, std::max(P, 1), y, oc, &n_out, ws, wsb, nullptr);
      if (rc) { fprintf(stderr, "rc %d %s\n", rc, g_err); return 2; }
      out.insert(out.end(), y, y + n_out); pos += P; free(pk);
    }
    if (pos - start != total) return 3;
    wr(argv[8], out.data(), out.size() * 4);
    free(st); free(ws); free(y);
  }
  free(filt);
  return 0;
}
