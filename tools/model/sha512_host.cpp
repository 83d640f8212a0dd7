// Host build of the SHA-512 / HMAC-SHA512 code (csrc/mpe_sha512.h under MPE_SHA512_HOST) for tests/test_bip32_cpu.py: the rounds, the
// message schedule, the padding and the HMAC's block loop are the header's text, the same the kernels compile (the rotations alone are
// plain shifts here, two alignbit operations on the device).
//   g++ -O2 -shared -fPIC -DMPE_SHA512_HOST -I multi_party_ecdsa_amd/csrc tools/model/sha512_host.cpp -o build/libsha512_host.so
// With -DSHA512_HOST_MAIN it is a stand-alone program for a sanitizer run (g++ -fsanitize=address,undefined):
//   sha512_host sha LEN | hmac KEYLEN LEN   prints the digest of the message byte i = 131 i + 7 (key byte i = 29 i + 3), in hex.
#include <string>
#include "mpe_sha512.h"

extern "C" {
void sha512h_digest(const uint8_t* msg, uint32_t len, uint8_t* out) { mpe::s512::sha512_item(msg, len, out); }
void sha512h_hmac(const uint8_t* key, uint32_t key_len, const uint8_t* msg, uint32_t len, uint8_t* out) {
  mpe::s512::hmac_sha512_item(key, key_len, msg, len, out);
}
}

#ifdef SHA512_HOST_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const bool mac = std::string(argv[1]) == "hmac";
  if (mac && argc < 4) return 2;
  const int key_len = mac ? atoi(argv[2]) : 0, len = atoi(argv[mac ? 3 : 2]);
  std::vector<uint8_t> key(key_len), msg(len);              // exact sizes: a read past the end is the sanitizer's to report
  for (int i = 0; i < key_len; ++i) key[i] = (uint8_t)(i * 29 + 3);
  for (int i = 0; i < len; ++i) msg[i] = (uint8_t)(i * 131 + 7);
  uint8_t out[64];
  if (mac) sha512h_hmac(key.data(), key_len, msg.data(), len, out);
  else sha512h_digest(msg.data(), len, out);
  for (int i = 0; i < 64; ++i) printf("%02x", out[i]);
  printf("\n");
  return 0;
}
#endif
