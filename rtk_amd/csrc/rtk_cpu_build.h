// rtk_cpu_build.h -- the CPU task-graph builder (rtk_cpu_build.cpp) as the rtk.h build API (rtk_build_api.hip) drives it, where the
// host selects it explicitly (rtk_amd_set_builder). Host only.
#pragma once

#include "rtk.h"

#include <stddef.h>

struct rtk_cpu_build;
void rtk_cpu_task_start(const rtk_task *, rtk_task_ctx *);
rtk_cpu_build *rtk_cpu_build_start(const rtk_scene_desc *desc, void *owner, rtk_task *first_task, rtk_task_fn *runner);
size_t rtk_cpu_build_run(rtk_cpu_build *b, const rtk_task *task, bool start, rtk_task *queue, size_t queue_size);
bool rtk_cpu_build_done(const rtk_cpu_build *b);
size_t rtk_cpu_build_size(rtk_cpu_build *b);
bool rtk_cpu_build_write(rtk_cpu_build *b, void *buffer, size_t size);
void rtk_cpu_build_free(rtk_cpu_build *b);
