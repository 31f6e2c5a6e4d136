# The dense-start driver on top of the sanitizer build of Makefile (same objects, same flags):
#   make -f dense_start.mk _build/dense_start
include Makefile

$(OUT)/dense_start.o: dense_start.cpp plan_emulate.h $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -O2 -x hip -c $< -o $@
$(OUT)/dense_start: $(OUT)/dense_start.o $(OUT)/plan_emulate.o $(OUT)/schedule.o $(OUT)/engine.o $(KERNEL_OBJS)
	$(HIPCC) $(SAN) $^ -o $@
