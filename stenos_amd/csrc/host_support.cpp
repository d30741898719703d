// host_support.cpp -- what the host stages lean on: zstd through dlopen and the worker threads of the zstd stages.
#include <dlfcn.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "host.h"

namespace stenos_host {

Zstd::Zstd()
{
	const char* names[] = { "/opt/conda/lib/libzstd.so.1", "libzstd.so.1", "libzstd.so", nullptr };
	void* h = nullptr;
	for (int i = 0; names[i] && !h; ++i)
		h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
	if (!h)
		return;
	compress_once = (zstd_compress_fn)dlsym(h, "ZSTD_compress");
	create_cctx = (zstd_createcctx_fn)dlsym(h, "ZSTD_createCCtx");
	free_cctx = (zstd_freecctx_fn)dlsym(h, "ZSTD_freeCCtx");
	compress_cctx = (zstd_compresscctx_fn)dlsym(h, "ZSTD_compressCCtx");
	if (!create_cctx || !free_cctx || !compress_cctx)
		create_cctx = nullptr;
	decompress = (zstd_decompress_fn)dlsym(h, "ZSTD_decompress");
	is_error = (zstd_iserror_fn)dlsym(h, "ZSTD_isError");
	max_level = (zstd_maxclevel_fn)dlsym(h, "ZSTD_maxCLevel");
	ok = compress_once && decompress && is_error && max_level;
}
Zstd& zstd()
{
	static Zstd z;
	return z;
}

// Host side worker threads for the zstd stages of levels >= 2 (one superblock per task).
#ifndef STENOS_HOST_THREADS_CAP
#define STENOS_HOST_THREADS_CAP 64
#endif
constexpr unsigned HOST_THREADS_DEFAULT_CAP = STENOS_HOST_THREADS_CAP; // workers of the strategy layer unless STENOS_HOST_THREADS says otherwise (at most 256)
static unsigned host_threads()
{
	static const unsigned threads = [] { // (read once: no environment look-ups on the call path)
		unsigned n = std::thread::hardware_concurrency();
		// a container's CPU quota (cgroup v2 cpu.max / v1 cfs quota) is what the workers really get: beyond about 1.5 x
		// of it more threads only take time slices from each other (measured on a 16-CPU share of a 256-thread host:
		// 24 workers 13.8 GB/s, 64: 11.5, 256: 4.7 for doubles at level 2)
		{
			double quota = 0, period = 0;
			if (FILE* fp = fopen("/sys/fs/cgroup/cpu.max", "r")) {
				char q[32] = { 0 };
				if (fscanf(fp, "%31s %lf", q, &period) == 2 && strcmp(q, "max") != 0)
					quota = atof(q);
				fclose(fp);
			}
			else if (FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
				if (fscanf(fq, "%lf", &quota) != 1)
					quota = 0;
				fclose(fq);
				if (FILE* fr = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
					if (fscanf(fr, "%lf", &period) != 1)
						period = 0;
					fclose(fr);
				}
			}
			if (quota > 0 && period > 0) {
				const unsigned share = (unsigned)(quota / period * 1.5 + 0.5);
				n = share < n ? (share < 1 ? 1u : share) : n;
			}
		}
		n = n > HOST_THREADS_DEFAULT_CAP ? HOST_THREADS_DEFAULT_CAP : n;
		if (const char* e = getenv("STENOS_HOST_THREADS"))
			if (atoi(e) > 0)
				n = (unsigned)atoi(e);
		return n > 256 ? 256u : n < 1 ? 1u : n;
	}();
	return threads;
}

// Persistent workers (created on first use, joined at unload): a batch of superblocks is a few milliseconds of
// work, too little to pay for 64 thread creations each time.  One job at a time; the caller works too.
class WorkerPool {
	std::vector<std::thread> threads_;
	std::mutex job_mutex_, m_;
	std::condition_variable cv_work_, cv_done_;
	const std::function<void(uint64_t)>* fn_ = nullptr;
	uint64_t cnt_ = 0, generation_ = 0;
	std::atomic<uint64_t> next_{ 0 };
	unsigned busy_ = 0, wanted_ = 0;
	bool stop_ = false;

	void drain()
	{
		for (uint64_t k; (k = next_.fetch_add(1)) < cnt_;)
			(*fn_)(k);
	}
	void loop(unsigned id)
	{
		uint64_t seen = 0;
		std::unique_lock<std::mutex> lk(m_);
		for (;;) {
			cv_work_.wait(lk, [&] { return stop_ || generation_ != seen; });
			if (stop_)
				return;
			seen = generation_;
			if (id >= wanted_)
				continue;
			lk.unlock();
			drain();
			lk.lock();
			if (--busy_ == 0)
				cv_done_.notify_one();
		}
	}

public:
	~WorkerPool()
	{
		{
			std::lock_guard<std::mutex> lk(m_);
			stop_ = true;
		}
		cv_work_.notify_all();
		for (auto& t : threads_)
			t.join();
	}
	void run(uint64_t cnt, const std::function<void(uint64_t)>& fn)
	{
		const unsigned nthreads = host_threads();
		const unsigned helpers = (unsigned)((cnt < nthreads ? cnt : nthreads) - (cnt ? 1 : 0));
		std::lock_guard<std::mutex> job(job_mutex_);
		if (helpers == 0) {
			for (uint64_t k = 0; k < cnt; ++k)
				fn(k);
			return;
		}
		{
			std::lock_guard<std::mutex> lk(m_);
			while (threads_.size() < helpers) {
				const unsigned id = (unsigned)threads_.size();
				threads_.emplace_back([this, id] { loop(id); });
			}
			fn_ = &fn;
			cnt_ = cnt;
			next_ = 0;
			wanted_ = helpers;
			busy_ = helpers;
			++generation_;
		}
		cv_work_.notify_all();
		drain();
		std::unique_lock<std::mutex> lk(m_);
		cv_done_.wait(lk, [&] { return busy_ == 0; });
	}
};

void parallel_for(uint64_t cnt, const std::function<void(uint64_t)>& fn)
{
	static WorkerPool pool;
	pool.run(cnt, fn);
}

} // namespace stenos_host
