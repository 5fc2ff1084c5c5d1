// set_arena.hpp -- where one hashing thread of `ganon-build --hash-sets packed|spilled` keeps the payload words of its files' packed sets
// (csrc/gn_packed_set.h): in memory, or in a file of its own that is appended to while hashing, mapped read-only for the passes of the
// fill -- clean, file-backed pages the kernel may drop and read again, so the process's anonymous memory does not grow with the input --
// and removed when the arena goes, which is when the command ends, on success and on every failure path.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <fcntl.h>
#include <stdexcept>
#include <string>
#include <sys/mman.h>
#include <unistd.h>
#include <vector>

namespace gnbuild
{

class SetArena
{
public:
    SetArena() = default; // in memory
    // in the file `path`, created here (an existing file of that name is not touched: the name carries the process id)
    explicit SetArena(const std::string& path) : path_(path)
    {
        fd_ = ::open(path.c_str(), O_RDWR | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
        if (fd_ < 0)
            throw std::runtime_error("--hash-sets spilled: cannot create " + path + " (" + std::strerror(errno) + ")");
    }
    SetArena(const SetArena&) = delete;
    SetArena& operator=(const SetArena&) = delete;
    ~SetArena()
    {
        if (map_)
            ::munmap(const_cast<uint64_t*>(map_), words_ * 8);
        if (fd_ >= 0)
        {
            ::close(fd_);
            ::unlink(path_.c_str());
        }
    }

    bool               spilled() const { return fd_ >= 0; }
    const std::string& path() const { return path_; }
    uint64_t           words() const { return words_; }

    // `n` words behind what the arena holds
    void append(const uint64_t* w, uint64_t n)
    {
        if (n == 0)
            return;
        if (fd_ < 0)
            mem_.insert(mem_.end(), w, w + n);
        else
            for (const char *p = reinterpret_cast<const char*>(w), *e = p + n * 8; p < e;)
            {
                const ssize_t k = ::write(fd_, p, (size_t)(e - p));
                if (k < 0 && errno == EINTR)
                    continue;
                if (k <= 0)
                    throw std::runtime_error("--hash-sets spilled: write error on " + path_ + " (" + std::strerror(k < 0 ? errno : ENOSPC) + ")");
                p += k;
            }
        words_ += n;
    }

    // the words, for the passes: nothing is appended after the first call
    const uint64_t* data()
    {
        if (fd_ < 0)
            return mem_.data();
        if (!map_ && words_)
        {
            void* m = ::mmap(nullptr, words_ * 8, PROT_READ, MAP_SHARED, fd_, 0);
            if (m == MAP_FAILED)
                throw std::runtime_error("--hash-sets spilled: cannot map " + path_ + " (" + std::strerror(errno) + ")");
            map_ = static_cast<const uint64_t*>(m);
        }
        return map_;
    }

private:
    // (the memory arena grows by doubling, allocate-copy-free: at k = w = 31, 1.4 GB an arena, the hashing lap is 2.5 s where raw sets
    // take 0.89 s and the file arena 0.88 s -- CHANGELOG; an anonymous mapping grown by mremap is the supposed remedy, not built)
    std::string           path_;
    int                   fd_ = -1;
    std::vector<uint64_t> mem_;
    const uint64_t* map_   = nullptr;
    uint64_t        words_ = 0;
};

} // namespace gnbuild
