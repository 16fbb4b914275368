// The sample-format argument of every entry point that takes one, WITHOUT a GPU: the product sources linked against
// hip_standins.inc (sample values are zero, everything the host decides is real), like ogg_stream_host.cpp.  Prints a trace of
// statuses, sample counts, element counts and capacity thresholds for one format; tests/test_host_f32_interleaved.py compares the
// trace of LW_FMT_F32_INTERLEAVED with that of LW_FMT_F32_PLANAR (same element size and counts) and checks the refused values.
//   usage: fmt_host packets.bin api                 (create / call with fmt -1 .. 4: one line per entry point and value)
//          fmt_host packets.bin batch FMT           (batch, ring of 3 slots, sharder of two logical shards on device 0)
//          fmt_host stream.ogg seq FMT [K]          (read_dec_packet to the end; K > 0: read-ahead of K packets)
//          fmt_host stream.ogg ahead FMT K          (read_dec_packets of K)
//          fmt_host stream.ogg skip FMT N           (skip_samples_linear N, then read_dec_packet to the end)
//   packets.bin: [u32 length][bytes] of the three header packets, then of the audio packets of one stream
#include "../../include/lewton_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_standins.inc"
#define KERNEL_HOST_NO_HIP_OK 1 // (lw_runtime.cpp is linked)
#include "kernel_host.hpp"

static std::vector<std::vector<uint8_t>> split_packets(const std::vector<uint8_t> &d)
{
	std::vector<std::vector<uint8_t>> out;
	for (size_t o = 0; o + 4 <= d.size();) {
		uint32_t n;
		memcpy(&n, d.data() + o, 4);
		o += 4;
		if (o + n > d.size())
			break;
		out.emplace_back(d.begin() + o, d.begin() + o + n);
		o += n;
	}
	return out;
}

static size_t cap_for(lw_ogg_stream *s)
{
	lw_ident_info info;
	lw_ident_get_info(lw_ogg_stream_ident(s), &info);
	return (size_t)info.audio_channels << info.blocksize_1;
}

static lw_ogg_stream *open_stream(const std::vector<uint8_t> &data)
{
	int err = 0;
	return lw_ogg_stream_open(lw_ogg_reader_open_memory(data.data(), data.size(), 0), 0, &err);
}

static void show(lw_ogg_stream *s, size_t n, int status)
{
	uint64_t gp = 0;
	const int has = lw_ogg_stream_last_absgp(s, &gp);
	printf("P %zu %d %s%llu\n", n, status, has ? "" : "-", (unsigned long long)(has ? gp : 0));
}

int main(int argc, char **argv)
{
	if (argc < 3)
		return 2;
	const std::vector<uint8_t> data = slurp(argv[1]);
	const std::string mode = argv[2];
	const int fmt = argc > 3 ? atoi(argv[3]) : 0;
	const unsigned long long arg = argc > 4 ? strtoull(argv[4], nullptr, 10) : 0;
	std::vector<uint8_t> out(4u << 20); // (large enough for every call below; each call is told its own capacity)
	if (mode == "api" || mode == "batch") {
		const auto pk = split_packets(data);
		if (pk.size() < 4)
			return 2;
		int err = 0;
		lw_ident *id = lw_read_header_ident(pk[0].data(), pk[0].size(), &err);
		lw_ident_info info;
		lw_ident_get_info(id, &info);
		lw_setup *setup = lw_read_header_setup(pk[2].data(), pk[2].size(), info.audio_channels, info.blocksize_0, info.blocksize_1, &err);
		lw_decoder *d = lw_decoder_create(id, setup, 0, &err);
		const int devs[2] = {0, 0};
		const size_t ch = info.audio_channels, cap = ch << info.blocksize_1;
		if (mode == "api") {
			for (int f = -1; f <= 4; f++) {
				lw_batch *b = lw_batch_create(d, 4, f, &err);
				printf("batch %d %d\n", f, err);
				lw_batch_destroy(b);
				lw_ring *r = lw_ring_create(d, 3, 4, f, &err);
				printf("ring %d %d\n", f, err);
				lw_ring_destroy(r);
				lw_sharder *sh = lw_sharder_create(id, setup, devs, 2, 4, f, &err);
				printf("sharder %d %d\n", f, err);
				lw_sharder_destroy(sh);
				lw_pwr *pw = lw_pwr_new(d);
				size_t m = 0;
				printf("packet %d %d\n", f, lw_read_audio_packet(d, pk[3].data(), pk[3].size(), pw, f, out.data(), cap, &m));
				lw_pwr_free(pw);
			}
		} else {
			const size_t n = pk.size() - 3;
			// batch: results, element count, the synth capacity threshold
			lw_batch *b = lw_batch_create(d, n, fmt, &err);
			lw_pwr *pw = lw_pwr_new(d);
			std::vector<lw_packet> in(n);
			for (size_t i = 0; i < n; i++)
				in[i] = lw_packet{pk[3 + i].data(), pk[3 + i].size(), pw};
			printf("B entropy %d\n", lw_batch_entropy(b, in.data(), n, 2));
			printf("B upload %d\n", lw_batch_upload(b, nullptr));
			const size_t el = lw_batch_out_elems(b);
			printf("B elems %zu\n", el);
			if (el)
				printf("B synth_short %d\n", lw_batch_synth_to_host(b, out.data(), el - 1, nullptr));
			printf("B synth %d\n", lw_batch_synth_to_host(b, out.data(), el, nullptr));
			const lw_packet_result *res = lw_batch_results(b);
			for (size_t i = 0; i < n; i++)
				printf("R %d %u %llu\n", res[i].status, res[i].n_samples, (unsigned long long)res[i].out_offset);
			lw_batch_destroy(b);
			// the single-packet call: capacity threshold per channel, then the packets
			lw_pwr_reset(pw);
			for (size_t i = 0; i < n; i++) {
				size_t m = 0;
				const int short_rc = lw_read_audio_packet(d, pk[3 + i].data(), pk[3 + i].size(), pw, fmt, out.data(), (size_t)1, &m);
				const int rc = lw_read_audio_packet(d, pk[3 + i].data(), pk[3 + i].size(), pw, fmt, out.data(), cap, &m);
				printf("S %d %d %zu\n", short_rc, rc, rc == LW_OK ? m : 0);
			}
			lw_pwr_free(pw);
			// ring of three slots
			lw_ring *r = lw_ring_create(d, 3, n, fmt, &err);
			lw_pwr *pr = lw_pwr_new(d);
			for (size_t i = 0; i < n; i++)
				in[i].pwr = pr;
			printf("G submit %d\n", lw_ring_submit(r, in.data(), n, 2));
			const lw_packet_result *rr = nullptr;
			const void *pcm = nullptr;
			size_t nr = 0, pe = 0;
			printf("G collect %d %zu %zu\n", lw_ring_collect(r, &rr, &nr, &pcm, &pe), nr, pe);
			for (size_t i = 0; i < nr; i++)
				printf("R %d %u %llu\n", rr[i].status, rr[i].n_samples, (unsigned long long)rr[i].out_offset);
			lw_ring_release(r);
			lw_ring_destroy(r);
			lw_pwr_free(pr);
			// sharder: two logical shards on device 0, two streams
			lw_sharder *sh = lw_sharder_create(id, setup, devs, 2, 2 * n, fmt, &err);
			lw_shard_stream *st[2] = {lw_sharder_stream_open(sh, 0), lw_sharder_stream_open(sh, 1)};
			std::vector<lw_shard_packet> sp;
			for (size_t i = 0; i < n; i++)
				for (int k = 0; k < 2; k++)
					sp.push_back(lw_shard_packet{st[k], pk[3 + i].data(), pk[3 + i].size()});
			std::vector<lw_packet_result> sr(sp.size());
			const size_t scap = out.size() / 4;
			printf("H decode %d\n", lw_sharder_decode(sh, sp.data(), sp.size(), 2, out.data(), scap, sr.data()));
			for (const auto &x : sr)
				printf("R %d %u %llu\n", x.status, x.n_samples, (unsigned long long)x.out_offset);
			lw_sharder_stream_close(st[0]);
			lw_sharder_stream_close(st[1]);
			lw_sharder_destroy(sh);
		}
		lw_decoder_destroy(d);
		lw_setup_free(setup);
		lw_ident_free(id);
		return 0;
	}
	lw_ogg_stream *s = open_stream(data);
	if (!s) {
		printf("E open\n");
		return 0;
	}
	const size_t cap = cap_for(s);
	if (mode == "seq") {
		if (arg)
			lw_ogg_stream_set_read_ahead(s, (size_t)arg, 2);
		for (;;) {
			size_t n = 0;
			const int short_rc = lw_ogg_stream_read_dec_packet(s, fmt, out.data(), cap - 1, &n); // (nothing is consumed)
			const int rc = lw_ogg_stream_read_dec_packet(s, fmt, out.data(), cap, &n);
			if (rc == LW_OGG_EOF) {
				printf("EOF %d\n", short_rc);
				break;
			}
			printf("C %d\n", short_rc);
			if (rc != LW_OK) {
				printf("E %d\n", rc);
				break;
			}
			show(s, n, 0);
		}
	} else if (mode == "ahead") {
		const size_t K = (size_t)std::max<unsigned long long>(1, arg);
		std::vector<uint32_t> ns(K);
		std::vector<int32_t> st(K);
		for (;;) {
			size_t np = 0;
			const int rc = lw_ogg_stream_read_dec_packets(s, fmt, K, 2, out.data(), cap * K, ns.data(), st.data(), &np);
			if (rc != LW_OK) {
				printf("E %d\n", rc);
				break;
			}
			printf("B %zu\n", np);
			for (size_t i = 0; i < np; i++)
				printf("Q %u %d\n", ns[i], st[i]);
			if (np == 0)
				break;
		}
	} else if (mode == "skip") {
		size_t left = (size_t)arg, n = 0;
		int got = 0;
		const int rc = lw_ogg_stream_skip_samples_linear(s, left, fmt, out.data(), cap, &n, &left, &got);
		printf("S %d %d %zu %zu\n", rc, got, got ? n : 0, left);
		for (;;) {
			const int r2 = lw_ogg_stream_read_dec_packet(s, fmt, out.data(), cap, &n);
			if (r2 != LW_OK) {
				printf("E %d\n", r2);
				break;
			}
			show(s, n, 0);
		}
	}
	lw_ogg_stream_close(s);
	return 0;
}
