// The guarded buffer of kernel_host.hpp held against AddressSanitizer itself: each mode makes ONE deliberate access of HOST memory
// on a shifted(64, OFF) buffer, and tests/test_host_kernel_harness.py asserts what came of it.  Built with the flags of every
// other host program (-fsanitize=address,undefined); no HIP code, no GPU.
//   kernel_host_selftest ok OFF      writes every byte of the buffer            "INTACT 1", exit 0
//   kernel_host_selftest slack OFF   stores one byte at at[-1]                  "INTACT 0", exit 0 for an OFF whose front has a remainder
//                                                                              that poisoning cannot express (OFF % 8 != 0); a report else
//   kernel_host_selftest front OFF   stores one byte at base[0]                 an AddressSanitizer report
//   kernel_host_selftest past OFF    loads the byte at at[64]                   an AddressSanitizer report
#define KERNEL_HOST_NO_HIP_OK 1
#include "kernel_host.hpp"

#include <string>

int main(int argc, char **argv)
{
	if (argc < 3)
		return 2;
	const std::string mode = argv[1];
	const unsigned off = (unsigned)atoi(argv[2]);
	const Guarded g = shifted(64, off);
	if (((uintptr_t)g.at & 15u) != (off & 15u))
		bad("the buffer starts %u bytes behind a 16-byte boundary, not %u", (unsigned)((uintptr_t)g.at & 15u), off & 15u);
	volatile char *at = g.at, *base = g.base; // (volatile: the accesses are made, and made as written)
	if (mode == "ok")
		for (int i = 0; i < 64; i++)
			at[i] = (char)i;
	else if (mode == "slack")
		at[-1] = 1;
	else if (mode == "front")
		base[0] = 1;
	else if (mode == "past")
		printf("READ %d\n", at[64]);
	else
		return 2;
	printf("INTACT %d\n", guard_intact(g) ? 1 : 0);
	free(g.base);
	return 0;
}
