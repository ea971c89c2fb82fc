// conceal_client.cpp - isvc_client.cpp's sibling for streams that have lost slices: a decoder application written against the
// ISVCDecoder interface that switches error concealment on the way the reference's console application does - through
// SetOption (DECODER_OPTION_ERROR_CON_IDC) after Initialize - and feeds one NAL unit per DecodeFrame2 call, then drains with
// (NULL, 0).  DecodeFrameNoDelay is not used: its second DecodeFrame2 call clears the buffer info of a concealed picture.
//
//   conceal_client in.264 out.yuv METHOD [SKIP]
//
// METHOD is the number of the ERROR_CON_IDC; -1 leaves the option alone.  The first SKIP delivered pictures are decoded and not
// written: tests/golden/make_conceal_streams.py puts other pictures in front of a damaged stream that way, to see which of the
// reference's concealed pictures depend on what its recycled picture buffers held.  One line per written picture on stdout:
// its index, the DECODING_STATE of the call that delivered it, its size.
//
// Built twice, like isvc_client.cpp: against the reference's own codec_api.h and libraries by make_conceal_streams.py (into
// oracle/_ref/, only where the reference lies), and against include/lh264_isvc.h + liblh264.so by tests/test_conceal_gpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#ifdef LH264_USE_REFERENCE_HEADER
#include "codec_api.h"
#else
#include "lh264_isvc.h"
#endif

static void write_plane (FILE* f, const unsigned char* p, int stride, int w, int h) {
  for (int y = 0; y < h; y++) fwrite (p + (size_t)y * stride, 1, (size_t)w, f);
}

static int g_seen = 0, g_skip = 0, g_written = 0;
static void emit (FILE* out, unsigned char** dst, const SBufferInfo& info, int state) {
  if (info.iBufferStatus != 1) return;
  if (g_seen++ < g_skip) return;
  const int w = info.UsrData.sSystemBuffer.iWidth, h = info.UsrData.sSystemBuffer.iHeight;
  write_plane (out, dst[0], info.UsrData.sSystemBuffer.iStride[0], w, h);
  write_plane (out, dst[1], info.UsrData.sSystemBuffer.iStride[1], w / 2, h / 2);
  write_plane (out, dst[2], info.UsrData.sSystemBuffer.iStride[1], w / 2, h / 2);
  printf ("pic %d state=0x%x %dx%d\n", g_written++, state, w, h);
}

int main (int argc, char** argv) {
  if (argc < 4) { fprintf (stderr, "usage: %s in.264 out.yuv METHOD [SKIP]\n", argv[0]); return 2; }
  int method = atoi (argv[3]);
  g_skip = argc > 4 ? atoi (argv[4]) : 0;
  FILE* in = fopen (argv[1], "rb");
  if (!in) { perror (argv[1]); return 2; }
  std::vector<unsigned char> bs;
  unsigned char tmp[65536]; size_t n;
  while ((n = fread (tmp, 1, sizeof (tmp), in)) > 0) bs.insert (bs.end(), tmp, tmp + n);
  fclose (in);
  FILE* out = fopen (argv[2], "wb");
  if (!out) { perror (argv[2]); return 2; }

  ISVCDecoder* dec = NULL;
  if (WelsCreateDecoder (&dec) || !dec) { fprintf (stderr, "WelsCreateDecoder failed\n"); return 1; }
  SDecodingParam param; memset (&param, 0, sizeof (param));
  param.eOutputColorFormat = videoFormatI420;
  param.uiTargetDqLayer = (unsigned char) - 1;
  param.eEcActiveIdc = ERROR_CON_DISABLE;
  param.sVideoProperty.size = sizeof (param.sVideoProperty);
  param.sVideoProperty.eVideoBsType = VIDEO_BITSTREAM_DEFAULT;
  const long irc = dec->Initialize (&param);
  if (irc) { fprintf (stderr, "Initialize failed: %ld\n", irc); WelsDestroyDecoder (dec); return 3; }
  if (method >= 0 && dec->SetOption (DECODER_OPTION_ERROR_CON_IDC, &method)) { fprintf (stderr, "SetOption (DECODER_OPTION_ERROR_CON_IDC, %d) refused\n", method); return 4; }

  int state_or = 0;
  size_t pos = 0;
  unsigned long long ts = 0;
  while (pos < bs.size()) {
    size_t next = pos + 3;
    for (; next + 3 <= bs.size(); next++)
      if (bs[next] == 0 && bs[next + 1] == 0 && (bs[next + 2] == 1 || (next + 3 < bs.size() && bs[next + 2] == 0 && bs[next + 3] == 1))) break;
    if (next + 3 > bs.size()) next = bs.size();
    unsigned char* dst[3] = {NULL, NULL, NULL};
    SBufferInfo info; memset (&info, 0, sizeof (info));
    info.uiInBsTimeStamp = ++ts;
    const int st = (int)dec->DecodeFrame2 (&bs[pos], (int) (next - pos), dst, &info);
    state_or |= st;
    emit (out, dst, info, st);
    pos = next;
  }
  for (;;) {      // end of stream: drain
    int eos = 1;
    dec->SetOption (DECODER_OPTION_END_OF_STREAM, &eos);
    unsigned char* dst[3] = {NULL, NULL, NULL};
    SBufferInfo info; memset (&info, 0, sizeof (info));
    const int st = (int)dec->DecodeFrame2 (NULL, 0, dst, &info);
    state_or |= st;
    if (info.iBufferStatus != 1) break;
    emit (out, dst, info, st);
  }
  printf ("pictures=%d state=0x%x\n", g_written, state_or);
  dec->Uninitialize();
  WelsDestroyDecoder (dec);
  fclose (out);
  return 0;
}
